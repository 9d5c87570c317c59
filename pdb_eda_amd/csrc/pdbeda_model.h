// pdbeda_model.h -- the way from the model to a map: the density of a list of Gaussian atoms on a map's grid, and the five sums that
// correlate two maps.  No reference counterpart; the contracts are spelled out at pdbeda_model_density and pdbeda_map_pair_moments in
// include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_model_tile             a workgroup of 256 per tile of PT_C x PT_R x PT_S STORED voxels (the partition's tile over ncrs, not over the
//                            unique box), one thread per voxel (c fastest).  The tile's xyz bounding box comes from its 8 corners, grown by
//                            the LARGEST radius; the atoms of the grid cells that box touches (the partition's counting sort, cell edge from
//                            the largest radius) are streamed through an LDS buffer of MD_STAGE atoms: coordinates, the radius, the square
//                            that rejects without a square root, and the n_terms amplitude / exponent pairs, every one an fp64 array of its
//                            own -- all lanes read the SAME atom, a broadcast without bank conflicts.  Every thread keeps ONE long long: a
//                            term amp * exp(-(expo * d2)) is rounded once to 2^-S and added as an integer, so neither the staging run, nor
//                            the cell, nor the order of the atom list changes a bit.  A tile with more atoms than one buffer runs the buffer
//                            again (uniform control flow).  The finish is fused: float32((double)sum * 2^-S) as rows of 64 bytes.
//   k_pair_moments           n and Sa, Sb, Saa, Sbb, Sab of two maps over the unique box where both voxels are finite and b > floor: a FIXED
//                            number of workgroups (from the box alone), lanes then waves in a fixed tree, one row of partials per workgroup.
//   k_pair_moments_fold      one block over the partials in index order (thread t takes rows t, t + 256, ...; then a fixed tree).
//
// The sphere test is the contract's sqrt(d2) <= (double)radius with IEEE sqrt.  The kernel takes the root only of pairs with d2 <= r2_hi =
// (r * r) (1 + 2^-50): sqrt_rn(d2) <= r implies d2 <= r^2 (1 + 2^-53)^2, and r * r is within 2^-53 of r^2, so r2_hi rejects no member.
#pragma once
#include "pdbeda_partition.h"

namespace pdbeda {

static constexpr int MD_STAGE = 256;                     // atoms of one LDS buffer: 6 KB of coordinates, 4 KB of radii, 24 KB of terms = 34 KB
static constexpr int MD_TERMS = PDBEDA_MODEL_MAX_TERMS;
static constexpr int PM_BLOCKS = 1024;                   // workgroups of k_pair_moments at the most (fewer for a box below 256 K voxels)

struct ModelArgs {
    const Geom *geom;                    // of the output map (= of `like`)
    int tiles_c, tiles_r;                // tiles along c and r (tile number = (ts * tiles_r + tr) * tiles_c + tc)
    CellGrid grid;
    const double *sorted;                // [gridded][3]
    const int *sorted_index;             // original atom index of each sorted point
    const unsigned *start;               // [n_cells + 1]
    const double *amp, *expo;            // [n_atoms][n_terms], the caller's order
    const float *radii;                  // [n_atoms]
    int n_terms;
    double r_max;                        // (double) of the largest radius
    double fix_mul, fix_inv;             // 2^S, 2^-S
    float *out;                          // [ns][nr][nc]
    unsigned long long *counters;        // [2]: the most atoms a tile staged (atomic max), tiles with more than one staging run
};

__global__ void __launch_bounds__(256) k_model_tile(ModelArgs a) {
    __shared__ double s_x[MD_STAGE], s_y[MD_STAGE], s_z[MD_STAGE];
    __shared__ double s_rad[MD_STAGE], s_r2[MD_STAGE];
    __shared__ double s_amp[MD_TERMS][MD_STAGE], s_expo[MD_TERMS][MD_STAGE];
    const int tid = threadIdx.x;
    const Geom &g = *a.geom;
    const int nc = g.ncrs[0], nr = g.ncrs[1], ns = g.ncrs[2];
    const int64_t tile = blockIdx.x;
    const int tc = (int)(tile % a.tiles_c), tr = (int)((tile / a.tiles_c) % a.tiles_r), ts = (int)(tile / ((int64_t)a.tiles_c * a.tiles_r));
    const int c0 = tc * PT_C, r0 = tr * PT_R, s0 = ts * PT_S;
    const int c = c0 + (tid & (PT_C - 1)), r = r0 + ((tid / PT_C) & (PT_R - 1)), s = s0 + tid / (PT_C * PT_R);
    const bool live = c < nc && r < nr && s < ns;

    // the cells the tile has to search: k_partition_tile's box of the 8 corners, grown by the largest radius and the same margins
    int lo[3], hi[3];
    bool any = true;
    {
        const int c1 = min(c0 + PT_C, nc) - 1, r1 = min(r0 + PT_R, nr) - 1, s1 = min(s0 + PT_S, ns) - 1;
        double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 8; ++k) {
            double p[3];
            crs2xyz(g, (k & 1) ? c1 : c0, (k & 2) ? r1 : r0, (k & 4) ? s1 : s0, p);
            for (int q = 0; q < 3; ++q) { blo[q] = fmin(blo[q], p[q]); bhi[q] = fmax(bhi[q], p[q]); }
        }
        for (int q = 0; q < 3; ++q) {
            const double pad = a.r_max * (1.0 + 1e-6) + 1e-9 * (fabs(blo[q]) + fabs(bhi[q]) + 1.0);
            const double fl = floor(((blo[q] - pad) - a.grid.lo[q]) / a.grid.edge), fh = floor(((bhi[q] + pad) - a.grid.lo[q]) / a.grid.edge);
            if (!(fh >= 0.0 && fl <= (double)(a.grid.dim[q] - 1))) any = false;      // (beside the grid, or NaN)
            lo[q] = fl < 0.0 ? 0 : (int)fmin(fl, (double)(a.grid.dim[q] - 1));
            hi[q] = fh > (double)(a.grid.dim[q] - 1) ? a.grid.dim[q] - 1 : (int)fmax(fh, 0.0);
        }
    }

    double p[3] = {0.0, 0.0, 0.0};
    if (live) crs2xyz(g, c, r, s, p);
    long long acc = 0;
    const int nt = a.n_terms;
    int fill = 0, runs = 0;
    long long staged = 0;
    // (uniform control flow: every thread walks the same rows and segments)
    auto gather = [&](int count) {
        __syncthreads();
        if (live)
            for (int k = 0; k < count; ++k) {
                const double dx = p[0] - s_x[k], dy = p[1] - s_y[k], dz = p[2] - s_z[k];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= s_r2[k])) continue;
                if (!(__dsqrt_rn(d2) <= s_rad[k])) continue;
                for (int j = 0; j < nt; ++j) {
                    const double e = s_expo[j][k] * d2;
                    const double t = s_amp[j][k] * exp(-e);
                    acc += fix_of(t, a.fix_mul);
                }
            }
        ++runs;
    };
    if (any && a.grid.n_cells > 0)
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y) {
                const int64_t row = ((int64_t)z * a.grid.dim[1] + y) * a.grid.dim[0];
                unsigned b = a.start[row + lo[0]];
                const unsigned e = a.start[row + hi[0] + 1];      // (cells lo[0]..hi[0] of a row are consecutive)
                staged += (long long)(e - b);
                while (b < e) {
                    const int take = (int)min((unsigned)(MD_STAGE - fill), e - b);
                    for (int i = tid; i < take; i += 256) {
                        const double *q = a.sorted + 3 * (size_t)(b + i);
                        const size_t at = (size_t)a.sorted_index[b + i];
                        const double rad = (double)a.radii[at];
                        s_x[fill + i] = q[0]; s_y[fill + i] = q[1]; s_z[fill + i] = q[2];
                        s_rad[fill + i] = rad;
                        s_r2[fill + i] = (rad * rad) * (1.0 + 0x1p-50);
                        for (int j = 0; j < nt; ++j) { s_amp[j][fill + i] = a.amp[at * nt + j]; s_expo[j][fill + i] = a.expo[at * nt + j]; }
                    }
                    fill += take;
                    b += (unsigned)take;
                    if (fill == MD_STAGE) {
                        gather(fill);
                        __syncthreads();      // (the buffer is written again)
                        fill = 0;
                    }
                }
            }
    if (fill > 0) gather(fill);
    if (live) a.out[((int64_t)s * nr + r) * nc + c] = (float)((double)acc * a.fix_inv);      // (a power of two: the product is exact; 0 -> +0.0f)
    if (tid == 0) {
        if (staged > 0) atomicMax(&a.counters[0], (unsigned long long)staged);
        if (runs > 1) atomicAdd(&a.counters[1], 1ull);
    }
}

// ---- the five sums of a pair of maps -----------------------------------------------------------------------------------------------------
// partials: [gridDim.x][6] doubles -- n (a count below 2^53 as a double: exact), Sa, Sb, Saa, Sbb, Sab.  Thread t of workgroup w takes the box voxels
// w * 256 + t, + gridDim.x * 256, ... in order; the lanes fold by xor shuffles, the waves as (0 + 1) + (2 + 3): one order for one grid size.
__global__ void __launch_bounds__(256) k_pair_moments(const float *__restrict__ a, const float *__restrict__ b, int n0, int n1, int uc, int ur, int us, double b_floor,
                                                      double *__restrict__ partials) {
    __shared__ double s_part[4][6];
    const int64_t total = (int64_t)uc * ur * us;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / uc, c = i - row * uc, s = row / ur, r = row - s * ur;
        const int64_t at = (s * n1 + r) * n0 + c;
        const double x = (double)a[at], y = (double)b[at];
        if (!(isfinite(x) && isfinite(y) && y > b_floor)) continue;
        v[0] += 1.0; v[1] += x; v[2] += y; v[3] += x * x; v[4] += y * y; v[5] += x * y;
    }
    for (int k = 0; k < 6; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; ++k) s_part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 6) partials[6 * (size_t)blockIdx.x + threadIdx.x] = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
}

// out: [6] doubles, n first.
__global__ void __launch_bounds__(256) k_pair_moments_fold(const double *__restrict__ partials, int n_rows, double *__restrict__ out) {
    __shared__ double s_part[6][256];
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_rows; i += 256)
        for (int k = 0; k < 6; ++k) v[k] += partials[6 * (size_t)i + k];
    for (int k = 0; k < 6; ++k) s_part[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 6; ++k) s_part[k][threadIdx.x] += s_part[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = s_part[threadIdx.x][0];
}

}  // namespace pdbeda
