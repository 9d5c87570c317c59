// pdbeda_qscore.h -- the map BETWEEN voxels: trilinear density at arbitrary coordinates, and per-atom Q-scores (Pintilie et al., Nature
// Methods 2020) that sample it on concentric spheres around every atom.  No reference counterpart; the contracts are spelled out at
// pdbeda_interp_density and pdbeda_atom_qscores in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   interp_trilinear     the eight corners around a fractional grid position through fetch_wrapped (periodic wrap, 0 where nothing is stored),
//                        promoted to fp64 and folded by lerp(a, b, t) = a + t * (b - a) along c, then r, then s.
//   k_interp_density     one thread per point.
//   k_atom_qscores       a wave of 64 per scored atom, four to a workgroup of 256.  The wave gathers into its LDS slice the atoms of the
//                        cells around its atom (the cell grid of pdbeda_cellgrid.h, edge > 2 R_max) that lie within 2 R_max of it -- the only
//                        atoms that can be nearer to a sample point than the atom itself -- as three fp64 arrays (every lane reads the SAME
//                        atom: a broadcast without bank conflicts).  Per shell and candidate level lane j owns candidate j: it tests its
//                        point against the staged atoms, a __ballot counts the accepted, and at the level the shell stops at the accepted
//                        lanes gather their eight corners; count, sums, min and max are folded with __shfl_xor (a butterfly: every lane
//                        ends with the same bits).  An atom with more than QS_STAGE neighbours walks the same cells in global memory for
//                        every candidate instead: slower, and as right.  One finish per wave.
//
// Nothing is accumulated across waves and no floating-point atomic is used: two runs agree to the bit, and the order of the atom list does
// not matter (acceptance is an "any" over the competitors).  The sums behind the correlation are taken on values shifted by the shell-0
// sample (the atom's own position, which every atom keeps) and by ref[0]: the one-pass variances then lose nothing to cancellation.
#pragma once
#include "pdbeda_partition.h"
#include "pdbeda_wave.h"

namespace pdbeda {

static constexpr int QS_STAGE = 128;      // neighbours a wave stages: 3 KB of coordinates a wave, 12 KB a workgroup (a protein has 30 to 40 atoms within 4 A)

// Corner values -> the interpolant: the fp32 corners are promoted first; c, then r, then s; t == 0 returns the base corner exactly whenever the
// other corner is finite (0 * finite = 0).  *valid: all eight corners are stored, whatever their weights.
// (Fetch: (c, r, s, bool *stored) -> float.  fetch_wrapped for the map itself; k_pose_scores reads a staged copy of the same floats and flags.)
template <typename Fetch>
__device__ inline double interp_trilinear_through(const Fetch &fetch, const double f[3], bool *valid) {
    const double fl[3] = {floor(f[0]), floor(f[1]), floor(f[2])};
    const int32_t b[3] = {(int32_t)fl[0], (int32_t)fl[1], (int32_t)fl[2]};
    const double t[3] = {f[0] - fl[0], f[1] - fl[1], f[2] - fl[2]};
    double v[8];
    bool all = true;
    for (int k = 0; k < 8; ++k) {
        bool ok;
        v[k] = (double)fetch(b[0] + (k & 1), b[1] + ((k >> 1) & 1), b[2] + (k >> 2), &ok);
        all = all && ok;
    }
    *valid = all;
    const double c00 = v[0] + t[0] * (v[1] - v[0]), c10 = v[2] + t[0] * (v[3] - v[2]);
    const double c01 = v[4] + t[0] * (v[5] - v[4]), c11 = v[6] + t[0] * (v[7] - v[6]);
    const double r0 = c00 + t[1] * (c10 - c00), r1 = c01 + t[1] * (c11 - c01);
    return r0 + t[2] * (r1 - r0);
}
__device__ inline double interp_trilinear(const Geom &g, const float *__restrict__ dens, const double f[3], bool *valid) {
    return interp_trilinear_through([&](int32_t c, int32_t r, int32_t s, bool *ok) { return fetch_wrapped(g, dens, c, r, s, ok); }, f, valid);
}

__global__ void __launch_bounds__(256) k_interp_density(const Geom *__restrict__ geom, const float *__restrict__ dens, const double *__restrict__ xyz, int64_t n,
                                                        double *__restrict__ out, uint8_t *__restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (the launch is not capped: one thread per point)
    if (i >= n) return;
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double f[3];
    xyz2frac(*geom, p, f);
    bool ok;
    const double v = interp_trilinear(*geom, dens, f, &ok);
    if (out) out[i] = v;
    if (valid) valid[i] = ok ? 1 : 0;
}

struct QScoreArgs {
    const Geom *geom;
    const float *dens;
    const double *xyz;                   // [n_all][3], the caller's order
    const int32_t *scored;               // [n_scored], or nullptr: all, in order
    int64_t n_scored;
    CellGrid grid;                       // over xyz, edge > reach
    const double *sorted;                // [gridded][3]
    const int *sorted_index;
    const unsigned *start;               // [n_cells + 1]
    double step, reach2;                 // reach = 2 R_max (1 + 1e-6): an atom farther than that from the scored atom wins no sample point
    int n_shells, n_levels, min_points;
    int level_off[PDBEDA_QSCORE_MAX_LEVELS + 1];
    const double *ref;                   // [n_shells]
    const double *unit;                  // [level_off[n_levels]][3]
    double *q;                           // [n_scored]
    int32_t *n_points;                   // [n_scored]
    int32_t *shell_n;                    // [n_scored][n_shells]
    double *shell_mean;                  // [n_scored][n_shells]
    uint8_t *valid;                      // [n_scored]
    unsigned long long *counters;        // [2]
};

__device__ inline double qs_d2(const double p[3], double x, double y, double z) {
    const double dx = p[0] - x, dy = p[1] - y, dz = p[2] - z;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(256) k_atom_qscores(QScoreArgs a) {
    __shared__ double s_x[4][QS_STAGE], s_y[4][QS_STAGE], s_z[4][QS_STAGE];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (the wave's number, as a scalar: what hangs on it -- the atom, its cells -- stays in SGPRs)
    const int64_t item = (int64_t)blockIdx.x * 4 + wv;
    const bool live = item < a.n_scored;      // (wave-uniform; a wave without an atom only keeps the barrier company)
    const Geom &g = *a.geom;
    const CellGrid &cg = a.grid;
    int self = 0;
    double at[3] = {0.0, 0.0, 0.0};
    int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
    int n_nb = 0;
    if (live) {
        self = a.scored ? a.scored[item] : (int)item;
        at[0] = a.xyz[3 * (int64_t)self]; at[1] = a.xyz[3 * (int64_t)self + 1]; at[2] = a.xyz[3 * (int64_t)self + 2];
        // the neighbours: every other atom (by index; an atom on the same coordinate is one) of the 27 cells around the atom within the reach
        if (grid_range(cg, at, lo, hi))
            for_each_cell_row(cg, a.start, lo, hi, [&](unsigned b, unsigned e) {
                for (unsigned k0 = b; k0 < e; k0 += 64) {
                    const unsigned k = k0 + (unsigned)lane;
                    bool near = false;
                    double x = 0.0, y2 = 0.0, z2 = 0.0;
                    if (k < e) {
                        x = a.sorted[3 * (size_t)k]; y2 = a.sorted[3 * (size_t)k + 1]; z2 = a.sorted[3 * (size_t)k + 2];
                        near = a.sorted_index[k] != self && qs_d2(at, x, y2, z2) <= a.reach2;
                    }
                    const unsigned long long m = __ballot(near);
                    const int pos = n_nb + __popcll(m & ((1ull << lane) - 1ull));
                    if (near && pos < QS_STAGE) { s_x[wv][pos] = x; s_y[wv][pos] = y2; s_z[wv][pos] = z2; }
                    n_nb += __popcll(m);
                }
                return false;
            });
        else { lo[0] = lo[1] = lo[2] = 0; hi[0] = hi[1] = hi[2] = -1; }
    }
    __syncthreads();      // (the one barrier: every wave reaches it; the slices are only read from here on)
    if (!live) return;
    const bool staged = n_nb <= QS_STAGE;
    if (lane == 0) {
        if (!staged) atomicAdd(&a.counters[0], 1ull);
        atomicMax(&a.counters[1], (unsigned long long)n_nb);
    }

    // shell 0: the atom's own position, always kept
    double f[3];
    bool ok0;
    xyz2frac(g, at, f);
    const double v0 = interp_trilinear(g, a.dens, f, &ok0);
    const double shift = isfinite(v0) ? v0 : 0.0, ref0 = a.ref[0];
    int total = 1, shells_kept = 1;
    bool all_valid = ok0, all_finite = isfinite(v0);
    double sx = v0 - shift, sxx = sx * sx, sy = 0.0, syy = 0.0, sxy = 0.0;      // x: sampled - shift, y: ref[k] - ref[0]
    double vmin = v0, vmax = v0, ymin = 0.0, ymax = 0.0;
    if (lane == 0) { a.shell_n[item * a.n_shells] = 1; a.shell_mean[item * a.n_shells] = v0; }

    for (int k = 1; k < a.n_shells; ++k) {
        const double R = (double)k * a.step;
        unsigned long long kept = 0ull;
        double p[3] = {0.0, 0.0, 0.0};
        for (int l = 0; l < a.n_levels; ++l) {
            const int cnt = a.level_off[l + 1] - a.level_off[l];
            bool acc = lane < cnt;
            if (acc) {
                const double *u = a.unit + 3 * (size_t)(a.level_off[l] + lane);
                p[0] = at[0] + R * u[0]; p[1] = at[1] + R * u[1]; p[2] = at[2] + R * u[2];
            }
            const double d_self = qs_d2(p, at[0], at[1], at[2]);      // (from p like the others, not R * R: coincident atoms tie to the bit)
            if (staged) {
#pragma unroll 4
                for (int j = 0; j < n_nb; ++j)      // (unrolled: four broadcast reads in flight instead of one LDS round trip per neighbour)
                    if (qs_d2(p, s_x[wv][j], s_y[wv][j], s_z[wv][j]) < d_self) acc = false;
            } else {
                for_each_cell_row(cg, a.start, lo, hi, [&](unsigned b, unsigned e) {
#pragma unroll 4
                    for (unsigned j = b; j < e; ++j)      // (every lane reads the same atom)
                        if (a.sorted_index[j] != self && qs_d2(p, a.sorted[3 * (size_t)j], a.sorted[3 * (size_t)j + 1], a.sorted[3 * (size_t)j + 2]) < d_self) acc = false;
                    return false;
                });
            }
            kept = __ballot(acc);
            if (__popcll(kept) >= a.min_points) break;      // (else the next level; the last level's accepted are kept, maybe none)
        }
        const int n_k = __popcll(kept);
        const bool mine = (kept >> lane) & 1ull;
        double v = 0.0;
        bool ok = true;
        if (mine) {
            xyz2frac(g, p, f);
            v = interp_trilinear(g, a.dens, f, &ok);
        }
        const double d = mine ? v - shift : 0.0;
        const double s_v = wave_fold<SegAdd>(mine ? v : 0.0), s_d = wave_fold<SegAdd>(d), s_dd = wave_fold<SegAdd>(d * d);
        const double mn = wave_fold<SegFmin>(mine ? v : INFINITY), mx = wave_fold<SegFmax>(mine ? v : -INFINITY);
        all_valid = all_valid && __ballot(mine && !ok) == 0ull;
        all_finite = all_finite && __ballot(mine && !isfinite(v)) == 0ull;
        if (n_k > 0) {
            const double y = a.ref[k] - ref0;
            total += n_k; ++shells_kept;
            sx += s_d; sxx += s_dd;
            sy += (double)n_k * y; syy += (double)n_k * (y * y); sxy += y * s_d;
            vmin = fmin(vmin, mn); vmax = fmax(vmax, mx);
            ymin = fmin(ymin, y); ymax = fmax(ymax, y);
        }
        if (lane == 0) {
            a.shell_n[item * a.n_shells + k] = n_k;
            a.shell_mean[item * a.n_shells + k] = n_k > 0 ? s_v / (double)n_k : 0.0;
        }
    }
    if (lane != 0) return;
    double q = NAN;
    if (total >= 2 && shells_kept >= 2 && all_finite && vmin != vmax && ymin != ymax) {
        const double n = (double)total;
        const double cov = sxy - sx * sy / n, vx = sxx - sx * sx / n, vy = syy - sy * sy / n;
        q = cov / (__dsqrt_rn(vx) * __dsqrt_rn(vy));
        q = q > 1.0 ? 1.0 : (q < -1.0 ? -1.0 : q);
    }
    a.q[item] = q;
    a.n_points[item] = total;
    a.valid[item] = all_valid ? 1 : 0;
}

}  // namespace pdbeda
