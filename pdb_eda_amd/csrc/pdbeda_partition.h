// pdbeda_partition.h -- nearest-atom partition of a map: every voxel of the non-repeating box header.uniqueNcrs goes to the atom
// nearest to it (within one maximum distance) or to nobody, and the density is summed per owner.  No reference counterpart; the
// contract is spelled out at pdbeda_map_partition in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_grid_scatter_indexed   the scatter of the contacts grid's counting sort (pdbeda_contacts.h: count, scan, scatter) that also
//                            keeps each point's ORIGINAL index: the tie rule (lowest atom index) needs it, and so do the rows.
//   k_partition_range        only for a map that holds NaN / infinite voxels (the map's own quantum is refused then): max finite |rho|
//                            of the box by an integer atomic max on the bit pattern.
//   k_partition_tile         a workgroup of 256 per tile of PT_C x PT_R x PT_S voxels, one thread per voxel (c fastest).  The tile's
//                            xyz bounding box comes from its 8 corners (crs2xyz is affine: right on skewed cells too), grown by the
//                            maximum distance; the atoms of the grid cells that box touches are streamed through an LDS buffer of
//                            PT_STAGE atoms (coordinates as three fp64 arrays: every lane reads the SAME atom, a broadcast without
//                            bank conflicts) and every lane keeps its best (d2, index) with the tie rule.  A tile whose atoms fit ONE
//                            buffer -- every tile of a protein at 3.5 A -- sums per staged atom in LDS (integers) and issues one global
//                            integer atomic per (atom, tile, column) that owns something; a tile with more atoms runs the buffer
//                            several times and sends each voxel's contribution to global memory itself: slower, and as right.
//   k_partition_finish       integers -> the caller's columns (sum = integer / 2^shift, exact), and the sum of squares of the unowned voxels
//                            folded from the per-workgroup partials in index order by one block.
//
// Density sums are integers in the map's fixed-point quantum (fix_of): addition commutes, so neither the order of the atomics nor
// the order of the atom list (apart from the tie rule) changes a bit of the result.  d2 = (dx*dx + dy*dy) + dz*dz is evaluated the
// same way for every (voxel, atom) whichever tile or buffer run meets the pair, so owners do not depend on the tiling.
#pragma once
#include "pdbeda_contacts.h"

namespace pdbeda {

static constexpr int PT_C = 16, PT_R = 4, PT_S = 4;      // 256 voxels: 64-byte rows, a neighbourhood of about (16 + 7) x 11 x 11 A at 1 A voxels and 3.5 A
static constexpr int PT_STAGE = 512;                     // atoms of one LDS buffer: 12 KB of coordinates, 2 KB of indices, 18 KB of sums

struct PartitionArgs {
    const Geom *geom;
    const float *dens;
    int uc, ur, us;                      // header.uniqueNcrs
    int tiles_c, tiles_r;                // tiles along c and r (tile number = (ts * tiles_r + tr) * tiles_c + tc)
    CellGrid grid;
    const double *sorted;                // [gridded][3]
    const int *sorted_index;             // original atom index of each sorted point
    const unsigned *start;               // [n_cells + 1]
    double max_distance, cutoff;
    double fix_mul;
    unsigned long long *atom_n;          // [3][n_atoms]: n, n_pos, n_neg
    unsigned long long *atom_sum;        // [3][n_atoms]: sum, sum_pos, sum_neg (two's complement fixed point)
    int64_t n_atoms;
    unsigned long long *unowned;         // [6]: n, n_pos, n_neg, sum, sum_pos, sum_neg
    double *tile_sq;                     // [n_tiles]: sum of squares of the tile's unowned voxels
    int32_t *owner;                      // box voxels, or nullptr
};

__global__ void __launch_bounds__(256) k_grid_scatter_indexed(const double *__restrict__ xyz, int64_t n, CellGrid g, unsigned *__restrict__ cursor,
                                                              double *__restrict__ sorted, int *__restrict__ sorted_index, int64_t room) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (grid_cropped(g, v)) continue;
        const unsigned pos = atomicAdd(&cursor[grid_cell(g, v)], 1u);
        if ((int64_t)pos < room) { sorted[3 * pos] = v[0]; sorted[3 * pos + 1] = v[1]; sorted[3 * pos + 2] = v[2]; sorted_index[pos] = (int)i; }
    }
}

// max finite |rho| over the box as the bit pattern of a non-negative double (ordered like the integers); *out starts at 0.
__global__ void __launch_bounds__(256) k_partition_range(const float *__restrict__ dens, int n0, int n1, int uc, int ur, int us, unsigned long long *out) {
    const int64_t total = (int64_t)uc * ur * us;
    double best = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / uc, c = i - row * uc, s = row / ur, r = row - s * ur;
        const double v = fabs((double)dens[(s * n1 + r) * n0 + c]);
        if (isfinite(v) && v > best) best = v;
    }
    for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0 && best > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(best));
}

__device__ inline long long wave_sum_ll(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(256) k_partition_tile(PartitionArgs a) {
    __shared__ double s_x[PT_STAGE], s_y[PT_STAGE], s_z[PT_STAGE];
    __shared__ int s_idx[PT_STAGE];
    __shared__ unsigned long long s_sum[3][PT_STAGE];
    __shared__ unsigned int s_cnt[3][PT_STAGE];
    __shared__ long long s_un[4][6];
    __shared__ double s_sq[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Geom &g = *a.geom;
    const int64_t tile = blockIdx.x;
    const int tc = (int)(tile % a.tiles_c), tr = (int)((tile / a.tiles_c) % a.tiles_r), ts = (int)(tile / ((int64_t)a.tiles_c * a.tiles_r));
    const int c0 = tc * PT_C, r0 = tr * PT_R, s0 = ts * PT_S;
    const int c = c0 + (tid & (PT_C - 1)), r = r0 + ((tid / PT_C) & (PT_R - 1)), s = s0 + tid / (PT_C * PT_R);
    const bool live = c < a.uc && r < a.ur && s < a.us;

    // the cells the tile has to search: its corners' bounding box, grown by the maximum distance and by a margin far above the rounding
    // of crs2xyz and of the distance (an interior voxel may leave the corners' box by an ulp; the cell of a point is monotonic in it)
    int lo[3], hi[3];
    bool any = true;
    {
        const int c1 = min(c0 + PT_C, a.uc) - 1, r1 = min(r0 + PT_R, a.ur) - 1, s1 = min(s0 + PT_S, a.us) - 1;
        double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 8; ++k) {
            double p[3];
            crs2xyz(g, (k & 1) ? c1 : c0, (k & 2) ? r1 : r0, (k & 4) ? s1 : s0, p);
            for (int q = 0; q < 3; ++q) { blo[q] = fmin(blo[q], p[q]); bhi[q] = fmax(bhi[q], p[q]); }
        }
        for (int q = 0; q < 3; ++q) {
            const double pad = a.max_distance * (1.0 + 1e-6) + 1e-9 * (fabs(blo[q]) + fabs(bhi[q]) + 1.0);
            const double fl = floor(((blo[q] - pad) - a.grid.lo[q]) / a.grid.edge), fh = floor(((bhi[q] + pad) - a.grid.lo[q]) / a.grid.edge);
            if (!(fh >= 0.0 && fl <= (double)(a.grid.dim[q] - 1))) any = false;      // (beside the grid, or NaN)
            lo[q] = fl < 0.0 ? 0 : (int)fmin(fl, (double)(a.grid.dim[q] - 1));
            hi[q] = fh > (double)(a.grid.dim[q] - 1) ? a.grid.dim[q] - 1 : (int)fmax(fh, 0.0);
        }
    }

    double p[3] = {0.0, 0.0, 0.0};
    if (live) crs2xyz(g, c, r, s, p);
    double best = INFINITY;
    int best_idx = 0x7fffffff, best_slot = -1;
    int fill = 0, runs = 0;
    // (uniform control flow: every thread walks the same rows and segments)
    auto search = [&](int count) {
        __syncthreads();
        if (live)
            for (int k = 0; k < count; ++k) {
                const double dx = p[0] - s_x[k], dy = p[1] - s_y[k], dz = p[2] - s_z[k];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const int idx = s_idx[k];
                if (d2 < best || (d2 == best && idx < best_idx)) { best = d2; best_idx = idx; best_slot = k; }
            }
        ++runs;
    };
    if (any && a.grid.n_cells > 0)
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y) {
                const int64_t row = ((int64_t)z * a.grid.dim[1] + y) * a.grid.dim[0];
                unsigned b = a.start[row + lo[0]];
                const unsigned e = a.start[row + hi[0] + 1];      // (cells lo[0]..hi[0] of a row are consecutive)
                while (b < e) {
                    const int take = (int)min((unsigned)(PT_STAGE - fill), e - b);
                    for (int i = tid; i < take; i += 256) {
                        const double *q = a.sorted + 3 * (size_t)(b + i);
                        s_x[fill + i] = q[0]; s_y[fill + i] = q[1]; s_z[fill + i] = q[2];
                        s_idx[fill + i] = a.sorted_index[b + i];
                    }
                    fill += take;
                    b += (unsigned)take;
                    if (fill == PT_STAGE) {
                        search(fill);
                        __syncthreads();      // (the buffer is written again)
                        fill = 0;
                    }
                }
            }
    const int full_runs = runs;
    if (fill > 0) search(fill);
    // one buffer held every atom of the tile: best_slot names the owner's row of the LDS sums
    const bool lds_sums = full_runs == 0 && fill > 0;
    if (lds_sums) {
        for (int k = tid; k < fill; k += 256) {
            s_cnt[0][k] = 0u; s_cnt[1][k] = 0u; s_cnt[2][k] = 0u;
            s_sum[0][k] = 0ull; s_sum[1][k] = 0ull; s_sum[2][k] = 0ull;
        }
        __syncthreads();
    }

    const bool owned = live && best_slot >= 0 && __dsqrt_rn(best) <= a.max_distance;
    long long un[6] = {0, 0, 0, 0, 0, 0};
    double sq = 0.0;
    if (live) {
        const double rho = (double)a.dens[((int64_t)s * g.ncrs[1] + r) * g.ncrs[0] + c];
        const bool fin = isfinite(rho);
        const bool pos = fin && rho > a.cutoff, neg = fin && rho < -a.cutoff;
        const long long F = fin ? fix_of(rho, a.fix_mul) : 0ll;
        if (a.owner) a.owner[((int64_t)s * a.ur + r) * a.uc + c] = owned ? best_idx : -1;
        if (!owned) {
            un[0] = 1; un[1] = pos; un[2] = neg; un[3] = F; un[4] = pos ? F : 0; un[5] = neg ? F : 0;
            sq = fin ? rho * rho : 0.0;
        } else if (lds_sums) {
            atomicAdd(&s_cnt[0][best_slot], 1u);
            if (fin) atomicAdd(&s_sum[0][best_slot], (unsigned long long)F);
            if (pos) { atomicAdd(&s_cnt[1][best_slot], 1u); atomicAdd(&s_sum[1][best_slot], (unsigned long long)F); }
            if (neg) { atomicAdd(&s_cnt[2][best_slot], 1u); atomicAdd(&s_sum[2][best_slot], (unsigned long long)F); }
        } else {
            const size_t n = (size_t)a.n_atoms, i = (size_t)best_idx;
            atomicAdd(&a.atom_n[i], 1ull);
            if (fin) atomicAdd(&a.atom_sum[i], (unsigned long long)F);
            if (pos) { atomicAdd(&a.atom_n[n + i], 1ull); atomicAdd(&a.atom_sum[n + i], (unsigned long long)F); }
            if (neg) { atomicAdd(&a.atom_n[2 * n + i], 1ull); atomicAdd(&a.atom_sum[2 * n + i], (unsigned long long)F); }
        }
    }
    // the unowned voxels of the workgroup: integers in any order, the squares in a fixed tree (lanes, then waves 0..3)
    for (int k = 0; k < 6; ++k) un[k] = wave_sum_ll(un[k]);
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if (lane == 0) {
        for (int k = 0; k < 6; ++k) s_un[wv][k] = un[k];
        s_sq[wv] = sq;
    }
    __syncthreads();
    if (tid < 6) {
        const long long t = (s_un[0][tid] + s_un[1][tid]) + (s_un[2][tid] + s_un[3][tid]);
        if (t != 0) atomicAdd(&a.unowned[tid], (unsigned long long)t);
    }
    if (tid == 6) a.tile_sq[tile] = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
    if (lds_sums) {      // (the barrier above is also behind every LDS atomic)
        const size_t n = (size_t)a.n_atoms;
        for (int k = tid; k < fill; k += 256) {
            if (s_cnt[0][k] == 0u) continue;
            const size_t i = (size_t)s_idx[k];
            atomicAdd(&a.atom_n[i], (unsigned long long)s_cnt[0][k]);
            if (s_sum[0][k]) atomicAdd(&a.atom_sum[i], s_sum[0][k]);
            if (s_cnt[1][k]) { atomicAdd(&a.atom_n[n + i], (unsigned long long)s_cnt[1][k]); atomicAdd(&a.atom_sum[n + i], s_sum[1][k]); }
            if (s_cnt[2][k]) { atomicAdd(&a.atom_n[2 * n + i], (unsigned long long)s_cnt[2][k]); atomicAdd(&a.atom_sum[2 * n + i], s_sum[2][k]); }
        }
    }
}

// Blocks 0 .. gridDim.x - 2: one thread per atom and column, integers -> the caller's columns.  The last block: the unowned totals, and the
// squares folded in index order (thread t takes tiles t, t + 256, ... in order; then a fixed tree over the 256 threads).
__global__ void __launch_bounds__(256) k_partition_finish(const unsigned long long *__restrict__ atom_n, const unsigned long long *__restrict__ atom_sum, int64_t n_atoms,
                                                          const unsigned long long *__restrict__ unowned, const double *__restrict__ tile_sq, int64_t n_tiles, double fix_inv,
                                                          long long *__restrict__ out_n, double *__restrict__ out_sum, long long *__restrict__ out_un, double *__restrict__ out_us) {
    if (blockIdx.x + 1 < gridDim.x) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 3 * n_atoms; i += (int64_t)(gridDim.x - 1) * 256) {
            out_n[i] = (long long)atom_n[i];
            out_sum[i] = (double)(long long)atom_sum[i] * fix_inv;      // (a power of two: the product is exact)
        }
        return;
    }
    __shared__ double s_part[256];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < n_tiles; i += 256) t += tile_sq[i];
    s_part[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_part[threadIdx.x] += s_part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        out_un[threadIdx.x] = (long long)unowned[threadIdx.x];
        out_us[threadIdx.x] = (double)(long long)unowned[3 + threadIdx.x] * fix_inv;
    }
    if (threadIdx.x == 0) out_us[3] = s_part[0];
}

}  // namespace pdbeda
