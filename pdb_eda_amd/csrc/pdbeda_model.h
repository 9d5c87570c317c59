// pdbeda_model.h -- the way from the model to a map: the density of a list of Gaussian atoms on a map's grid, and the five sums that
// correlate two maps.  No reference counterpart; the contracts are spelled out at pdbeda_model_density and pdbeda_map_pair_moments in
// include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_model_tile             a workgroup of 256 per tile of PT_C x PT_R x PT_S STORED voxels (the partition's tile over ncrs, not over the
//                            unique box), one thread per voxel (c fastest).  The atoms of the grid cells within the LARGEST radius of the
//                            tile (pdbeda_cellgrid.h: tile_voxel, tile_cell_range, stage_cell_rows; the cell edge comes from that radius)
//                            are streamed through an LDS buffer of MD_STAGE atoms: coordinates, the radius, the square
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
    const int nc = g.ncrs[0], nr = g.ncrs[1];
    const TileVoxel tv = tile_voxel<PT_C, PT_R, PT_S>(blockIdx.x, a.tiles_c, a.tiles_r, g.ncrs, tid);
    const int c = tv.c, r = tv.r, s = tv.s;
    const bool live = tv.live;
    int lo[3], hi[3];
    const bool any = tile_cell_range(g, a.grid, tv.c0, tv.c1, a.r_max, lo, hi);

    double p[3] = {0.0, 0.0, 0.0};
    if (live) crs2xyz(g, c, r, s, p);
    long long acc = 0;
    const int nt = a.n_terms;
    const StageReport rep = !any ? StageReport{0, 0, 0} : stage_cell_rows<MD_STAGE>(a.grid, a.start, lo, hi, [&](int slot, unsigned k) {
        const double *q = a.sorted + 3 * (size_t)k;
        const size_t at = (size_t)a.sorted_index[k];
        const double rad = (double)a.radii[at];
        s_x[slot] = q[0]; s_y[slot] = q[1]; s_z[slot] = q[2];
        s_rad[slot] = rad;
        s_r2[slot] = (rad * rad) * (1.0 + 0x1p-50);
        for (int j = 0; j < nt; ++j) { s_amp[j][slot] = a.amp[at * nt + j]; s_expo[j][slot] = a.expo[at * nt + j]; }
    }, [&](int count) {
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
    });
    if (live) a.out[((int64_t)s * nr + r) * nc + c] = (float)((double)acc * a.fix_inv);      // (a power of two: the product is exact; 0 -> +0.0f)
    if (tid == 0) {
        if (rep.staged > 0) atomicMax(&a.counters[0], (unsigned long long)rep.staged);
        if (rep.runs > 1) atomicAdd(&a.counters[1], 1ull);
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
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);      // (wave_fold's order; rolled: the kernel is slower with six unrolled folds)
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
