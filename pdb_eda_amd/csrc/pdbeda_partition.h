// pdbeda_partition.h -- nearest-atom partition of a map: every voxel of the non-repeating box header.uniqueNcrs goes to the atom
// nearest to it (within one maximum distance) or to nobody, and the density is summed per owner.  No reference counterpart; the
// contract is spelled out at pdbeda_map_partition in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_partition_range        only for a map that holds NaN / infinite voxels (the map's own quantum is refused then): max finite |rho|
//                            of the box by an integer atomic max on the bit pattern.
//   k_partition_tile         a workgroup of 256 per tile of PT_C x PT_R x PT_S voxels, one thread per voxel (c fastest).  The atoms of
//                            the grid cells within the maximum distance of the tile (pdbeda_cellgrid.h: tile_voxel, tile_cell_range,
//                            stage_cell_rows; the atoms were sorted with their ORIGINAL index, which the tie rule and the rows need)
//                            are streamed through an LDS buffer of PT_STAGE atoms (coordinates as three fp64 arrays: every lane
//                            reads the SAME atom, a broadcast without bank conflicts) and every lane keeps its best (d2, index) with
//                            the tie rule.  A tile whose atoms fit ONE buffer -- every tile of a protein at 3.5 A -- sums per staged
//                            atom in LDS (integers) and issues one global integer atomic per (atom, tile, column) that owns something;
//                            a tile with more atoms runs the buffer several times and sends each voxel's contribution to global memory itself.
//   k_partition_finish       integers -> the caller's columns (sum = integer / 2^shift, exact), and the sum of squares of the unowned voxels
//                            folded from the per-workgroup partials in index order by one block.
//
// Density sums are integers in the map's fixed-point quantum (fix_of): addition commutes, so neither the order of the atomics nor
// the order of the atom list (apart from the tie rule) changes a bit of the result.  d2 = (dx*dx + dy*dy) + dz*dz is evaluated the
// same way for every (voxel, atom) whichever tile or buffer run meets the pair, so owners do not depend on the tiling.
#pragma once
#include "pdbeda_contacts.h"
#include "pdbeda_wave.h"

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

// max finite |rho| over the box as the bit pattern of a non-negative double (ordered like the integers); *out starts at 0.
__global__ void __launch_bounds__(256) k_partition_range(const float *__restrict__ dens, int n0, int n1, int uc, int ur, int us, unsigned long long *out) {
    const int64_t total = (int64_t)uc * ur * us;
    double best = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / uc, c = i - row * uc, s = row / ur, r = row - s * ur;
        const double v = fabs((double)dens[(s * n1 + r) * n0 + c]);
        if (isfinite(v) && v > best) best = v;
    }
    best = wave_fold<SegFmax>(best);
    if ((threadIdx.x & 63) == 0 && best > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(best));
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
    const int box[3] = {a.uc, a.ur, a.us};
    const TileVoxel tv = tile_voxel<PT_C, PT_R, PT_S>(tile, a.tiles_c, a.tiles_r, box, tid);
    const int c = tv.c, r = tv.r, s = tv.s;
    const bool live = tv.live;
    int lo[3], hi[3];
    const bool any = tile_cell_range(g, a.grid, tv.c0, tv.c1, a.max_distance, lo, hi);

    double p[3] = {0.0, 0.0, 0.0};
    if (live) crs2xyz(g, c, r, s, p);
    double best = INFINITY;
    int best_idx = 0x7fffffff, best_slot = -1;
    const StageReport rep = !any ? StageReport{0, 0, 0} : stage_cell_rows<PT_STAGE>(a.grid, a.start, lo, hi, [&](int slot, unsigned k) {
        const double *q = a.sorted + 3 * (size_t)k;
        s_x[slot] = q[0]; s_y[slot] = q[1]; s_z[slot] = q[2];
        s_idx[slot] = a.sorted_index[k];
    }, [&](int count) {
        __syncthreads();
        if (live)
            for (int k = 0; k < count; ++k) {
                const double dx = p[0] - s_x[k], dy = p[1] - s_y[k], dz = p[2] - s_z[k];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const int idx = s_idx[k];
                if (d2 < best || (d2 == best && idx < best_idx)) { best = d2; best_idx = idx; best_slot = k; }
            }
    });
    // one buffer held every atom of the tile: best_slot names the owner's row of the LDS sums
    const int fill = rep.last;
    const bool lds_sums = rep.runs == 1 && fill > 0;
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
    for (int k = 0; k < 6; ++k) un[k] = wave_fold<SegAdd>(un[k]);
    sq = wave_fold<SegAdd>(sq);
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
