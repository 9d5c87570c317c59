// pdbeda_basins.h -- peak basins: the significant voxels of the non-repeating box header.uniqueNcrs divided among the peaks of a
// peak list by steepest ascent, with per-basin sums and the highest pass to an adjacent basin.  No reference counterpart; the
// contract is spelled out at pdbeda_peaklist_basins in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_basin_parent    the peak stencil's tile (64 x 8 x 8 voxels plus a one-voxel halo in LDS, a wave per 256-byte row): threshold
//                     and ballot first; for the survivors the winner of the closed neighbourhood among the significant voxels, stored
//                     as a box position in the int32 volume `up` (-1 for an insignificant voxel).
//   k_basin_jump      one round of pointer doubling, up[v] = up[up[v]], in place: every value ever stored at v is an ancestor of v and
//                     the stores are aligned 32-bit words, so a reader that meets a newer value only jumps further.  A round that
//                     changed something raises its own flag; a round behind one that changed nothing returns at once; the host reads
//                     the flags of a batch of rounds in one wait.
//   k_basin_mark      one thread per peak of the list: up[voxel of peak i] = -2 - i.
//   k_basin_resolve   every significant voxel takes its root's mark (-2 - i); a voxel whose root carries none -- a root beside a NaN,
//                     which the peak rule lets nothing beat -- is an orphan: -1, and counted.  In place: a listed root's word does
//                     not change any more, an orphan root's word reads as "no mark" before and after its own thread rewrote it.
//   k_basin_sums      one pass over the tiles with the resolved volume (and its halo) in LDS: per voxel its count, quantised density
//                     and the saddle key of its pairs -- the density of a neighbour is read only where the neighbour lies in another
//                     basin; runs of equal basins along a wave row are combined by a segmented scan and the last lane of a run
//                     issues the integer atomics.
//   k_basin_decode    -2 - i  ->  i for the caller's volume (only when it is asked for).
//
// Every accumulator is an integer (counts, fixed-point sums, offset sums, a 64-bit maximum), so the order the atomics land in
// cannot change a bit.  No kernel here waits for another workgroup.
#pragma once
#include "pdbeda_kernels.h"
#include "pdbeda_wave.h"

namespace pdbeda {

static constexpr int BN_ACC = 12;            // accumulator columns per peak: n, sum |F|, s1[3], sw1 limbs [3][2], saddle key
static constexpr int BN_MAX_ROUNDS = 31;     // doubling reaches the root of any path shorter than 2^31
static constexpr int BN_BATCH = 8;           // rounds enqueued per wait

struct BasinArgs {
    const float *dens;
    int32_t *up;                             // box voxels [us][ur][uc]
    int32_t uc, ur, us;                      // header.uniqueNcrs
    int32_t nc, nr;                          // stored row / section pitch (header.ncrs)
    float cut;
    int32_t sign;
    const int32_t *peak_box;                 // [n_peaks]: box position of peak i
    int64_t n_peaks;
    unsigned long long *acc;                 // [BN_ACC][n_peaks]
    unsigned long long *orphans;
    double fix_mul;
};

// halo_stage (pdbeda_wave.h) once more, as a function of this header with one caller per instantiation: on the shared, force-inlined one
// k_basin_parent took 26 VGPRs for 20 and ran 0.9 % slower, k_basin_sums 2.5 % slower.  Keep the two bodies alike.
template <typename T>
__device__ inline void basin_stage(T (*tile)[PK_HR][PK_HC], const T *__restrict__ src, int64_t pitch_c, int64_t pitch_r, int c0, int r0, int s0,
                                   int uc, int ur, int us, T outside) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WAVES = PK_THREADS / 64, ROWS_PER_WAVE = PK_HS * PK_HR / WAVES, BATCH = 5;
    static_assert(PK_HS * PK_HR % WAVES == 0 && ROWS_PER_WAVE % BATCH == 0, "the halo rows divide among the waves in whole batches");
    for (int b = 0; b < ROWS_PER_WAVE; b += BATCH) {
        T v[BATCH], w[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int row = wave + WAVES * (b + k);
            const int hs = row / PK_HR, hr = row - hs * PK_HR;
            const int s = s0 - 1 + hs, r = r0 - 1 + hr;
            const bool row_in = (unsigned)s < (unsigned)us && (unsigned)r < (unsigned)ur;   // wave-uniform
            const T *p = src + ((int64_t)(row_in ? s : 0) * pitch_r + (row_in ? r : 0)) * pitch_c;
            const int c = c0 - 1 + lane, c2 = c0 + 63 + lane;
            v[k] = (row_in && (unsigned)c < (unsigned)uc) ? p[c] : outside;
            w[k] = (lane < 2 && row_in && c2 < uc) ? p[c2] : outside;
        }
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
            const int row = wave + WAVES * (b + k);
            const int hs = row / PK_HR, hr = row - hs * PK_HR;
            tile[hs][hr][lane] = v[k];
            if (lane < 2) tile[hs][hr][64 + lane] = w[k];
        }
    }
}

__device__ inline bool basin_pass(float v, float cut, int sign) { return sign > 0 ? v >= cut : v <= cut; }     // (a NaN fails)
__device__ inline uint32_t basin_mag(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__global__ __launch_bounds__(PK_THREADS) void k_basin_parent(BasinArgs a) {
    __shared__ float tile[PK_HS][PK_HR][PK_HC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * PK_C, r0 = blockIdx.y * PK_R, s0 = blockIdx.z * PK_S;
    const int uc = a.uc, ur = a.ur, us = a.us;
    // outside the box: NaN, which fails the threshold test, so the bounds of the box need no test of their own below
    basin_stage<float>(tile, a.dens, a.nc, a.nr, c0, r0, s0, uc, ur, us, __uint_as_float(0x7fc00000u));
    __syncthreads();
    const int c = c0 + lane;
    for (int q = wave; q < PK_R * PK_S; q += PK_THREADS / 64) {
        const int ss = q / PK_R, rr = q - ss * PK_R;
        const int r = r0 + rr, s = s0 + ss;
        if (r >= ur || s >= us) continue;                 // wave-uniform
        const float v = tile[ss + 1][rr + 1][lane + 1];
        const bool pass = c < uc && basin_pass(v, a.cut, a.sign);
        int32_t parent = -1;
        if (__ballot(pass) != 0ull && pass) {
            // the candidates in c-major order of their offsets, the voxel itself among them: a later one wins on a strictly
            // greater |D| only, so of equal candidates the c-major-first stays
            uint32_t best = 0u;
            int bc = 0, br = 0, bs = 0;
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc)
#pragma unroll
                for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                    for (int ds = -1; ds <= 1; ++ds) {
                        const float nb = tile[ss + 1 + ds][rr + 1 + dr][lane + 1 + dc];
                        const uint32_t mag = basin_mag(nb);
                        if (basin_pass(nb, a.cut, a.sign) && mag > best) { best = mag; bc = dc; br = dr; bs = ds; }
                    }
            parent = (int32_t)(((int64_t)(s + bs) * ur + (r + br)) * uc + (c + bc));
        }
        if (c < uc) a.up[((int64_t)s * ur + r) * uc + c] = parent;
    }
}

__global__ __launch_bounds__(256) void k_basin_jump(int32_t *up, int64_t n, const uint32_t *prev, uint32_t *changed) {
    if (prev && *prev == 0u) return;                      // the round before this one changed nothing (its kernel is done): neither would this
    bool any = false;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = up[v];
        if (x < 0) continue;
        const int32_t y = up[x];
        if (y != x) { up[v] = y; any = true; }
    }
    if (__ballot(any) != 0ull && (threadIdx.x & 63) == 0) *changed = 1u;
}

__global__ __launch_bounds__(256) void k_basin_mark(int32_t *up, const int32_t *__restrict__ peak_box, int64_t n_peaks) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_peaks; i += (int64_t)gridDim.x * blockDim.x)
        up[peak_box[i]] = (int32_t)(-2 - i);
}

__global__ __launch_bounds__(256) void k_basin_resolve(int32_t *up, int64_t n, unsigned long long *orphans) {
    unsigned lost = 0u;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = up[v];
        if (x < 0) continue;                              // insignificant, or a listed root
        const int32_t t = up[x];
        const int32_t res = t <= -2 ? t : -1;
        lost += res == -1 ? 1u : 0u;
        up[v] = res;
    }
    if (__ballot(lost != 0u) == 0ull) return;             // (every map without a NaN)
    lost = wave_fold<SegAdd>(lost);
    if ((threadIdx.x & 63) == 0) atomicAdd(orphans, (unsigned long long)lost);
}

// Inclusive sum over the lanes of a run: `head` is the first lane of this lane's run.  (seg_scan of pdbeda_wave.h names a run by an id and asks
// with a shuffle per distance; on a form of it that took this predicate k_basin_sums ran 2.5 % slower.)
template <typename T>
__device__ inline T basin_seg_sum(T v, int lane, int head) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane - off >= head) v += t;
    }
    return v;
}
__device__ inline unsigned long long basin_seg_max(unsigned long long v, int lane, int head) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(v, off, 64);
        if (lane - off >= head && t > v) v = t;
    }
    return v;
}

__device__ inline void basin_add_limbs(unsigned long long *lo, unsigned long long *hi, __int128 v) {
    long long l, h;
    fix_limbs(v, l, h);
    if (l) atomicAdd(lo, (unsigned long long)l);
    if (h) atomicAdd(hi, (unsigned long long)h);
}

__global__ __launch_bounds__(PK_THREADS) void k_basin_sums(BasinArgs a) {
    __shared__ int32_t mark[PK_HS][PK_HR][PK_HC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * PK_C, r0 = blockIdx.y * PK_R, s0 = blockIdx.z * PK_S;
    const int uc = a.uc, ur = a.ur, us = a.us;
    basin_stage<int32_t>(mark, a.up, uc, ur, c0, r0, s0, uc, ur, us, -1);
    __syncthreads();
    const size_t np = (size_t)a.n_peaks;
    for (int q = wave; q < PK_R * PK_S; q += PK_THREADS / 64) {
        const int ss = q / PK_R, rr = q - ss * PK_R;
        const int r = r0 + rr, s = s0 + ss;
        if (r >= ur || s >= us) continue;                 // wave-uniform
        const int32_t me = mark[ss + 1][rr + 1][lane + 1];
        const bool mine = me <= -2;
        if (__ballot(mine) == 0ull) continue;             // wave-uniform: most rows at 3 sigma
        unsigned long long key = 0ull;
        long long F = 0;
        if (mine) {                                       // (a marked voxel lies inside the box)
            const float *at = a.dens + ((int64_t)s * a.nr + r) * a.nc + (c0 + lane);
            const float v = *at;
            const double rho = (double)v;
            if (isfinite(rho)) { F = fix_of(rho, a.fix_mul); F = F < 0 ? -F : F; }
            const uint32_t mag = basin_mag(v);
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc)
#pragma unroll
                for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                    for (int ds = -1; ds <= 1; ++ds) {
                        const int32_t other = mark[ss + 1 + ds][rr + 1 + dr][lane + 1 + dc];
                        if (other > -2 || other == me) continue;
                        const uint32_t m2 = basin_mag(at[((int64_t)ds * a.nr + dr) * a.nc + dc]);      // (marked: inside the box)
                        const unsigned long long k = ((unsigned long long)(m2 < mag ? m2 : mag) << 32) | (unsigned long long)(~(uint32_t)(-2 - other));
                        key = k > key ? k : key;
                    }
        }
        // runs of equal marks along the row
        const int32_t left = __shfl_up(me, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || left != me);
        const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0ull;
        const int cnt = lane - head + 1;
        const int sum_lane = basin_seg_sum<int>(lane, lane, head);
        const long long W = basin_seg_sum<long long>(F, lane, head);
        const long long WL = basin_seg_sum<long long>(F * lane, lane, head);
        key = basin_seg_max(key, lane, head);
        if (!mine || !last) continue;
        const size_t i = (size_t)(-2 - me);
        const int32_t pos = a.peak_box[i];
        const int32_t pc = pos % uc, prs = pos / uc, pr = prs % ur, ps = prs / ur;
        const long long dc0 = (long long)c0 - pc, dr = (long long)r - pr, ds = (long long)s - ps;
        unsigned long long *acc = a.acc + i;
        atomicAdd(acc, (unsigned long long)cnt);
        if (W) atomicAdd(acc + np, (unsigned long long)W);
        const long long s1c = (long long)cnt * dc0 + sum_lane, s1r = (long long)cnt * dr, s1s = (long long)cnt * ds;
        if (s1c) atomicAdd(acc + 2 * np, (unsigned long long)s1c);
        if (s1r) atomicAdd(acc + 3 * np, (unsigned long long)s1r);
        if (s1s) atomicAdd(acc + 4 * np, (unsigned long long)s1s);
        if (W) {
            basin_add_limbs(acc + 5 * np, acc + 6 * np, (__int128)W * dc0 + WL);
            basin_add_limbs(acc + 7 * np, acc + 8 * np, (__int128)W * dr);
            basin_add_limbs(acc + 9 * np, acc + 10 * np, (__int128)W * ds);
        }
        if (key) atomicMax(acc + 11 * np, key);
    }
}

__global__ __launch_bounds__(256) void k_basin_decode(int32_t *up, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t x = up[v];
        if (x <= -2) up[v] = -2 - x;
    }
}

}  // namespace pdbeda
