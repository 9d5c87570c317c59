// pdbeda_wave.h -- the wave-level building blocks of the feature kernels (gfx950, wave64): folds, scans, segmented scans over the 64 lanes of a
// wave and the staging of a 64 x 8 x 8 tile with its halo.  Device only.  One definition of each: the order of
// the shuffles and of the operands below IS the summation and tie order of every kernel that calls them.  The folds, the
// scans, the operations and halo_stage are __forceinline__: a primitive that two kernels share is otherwise kept as a real function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdbeda {

// ---- operations: op(mine, the other lane's); SegMax / SegMin take the other's on a tie or an unordered pair, SegMaxMine keeps mine ----
struct SegAdd { template <typename T> __device__ __forceinline__ static T op(T a, T b) { return a + b; } };
struct SegMax { template <typename T> __device__ __forceinline__ static T op(T a, T b) { return a > b ? a : b; } };
struct SegMin { template <typename T> __device__ __forceinline__ static T op(T a, T b) { return a < b ? a : b; } };
struct SegMaxMine { template <typename T> __device__ __forceinline__ static T op(T a, T b) { return b > a ? b : a; } };      // mine stays on a tie or an unordered pair
// ... of doubles with IEEE minNum / maxNum: a NaN loses against a number
struct SegFmin { __device__ __forceinline__ static double op(double a, double b) { return fmin(a, b); } };
struct SegFmax { __device__ __forceinline__ static double op(double a, double b) { return fmax(a, b); } };

// ---- folds -----------------------------------------------------------------------------------------------------------------------------
// Butterfly over the 64 lanes, partner distances 32, ..., 1: every lane ends with the same bits.
template <typename Op, typename T> __device__ __forceinline__ T wave_fold(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::op(v, __shfl_xor(v, off, 64));
    return v;
}
// The tree whose result is read in lane 0 (the other lanes end with partial folds): distances 32, ..., 1, the lower lane's value on the left.
template <typename Op, typename T> __device__ __forceinline__ void wave_fold_down(T &v) {      // in place: on a copy the compiler orders the callers' code differently
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::op(v, __shfl_down(v, off));
}

// ---- scans -----------------------------------------------------------------------------------------------------------------------------
// Inclusive Hillis-Steele sum over the lanes of a wave, distances 1, 2, ..., 32: lane l ends with x[0] + ... + x[l], added in that tree.
template <typename T> __device__ __forceinline__ T wave_incl_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// ---- segmented scan --------------------------------------------------------------------------------------------------------------------
// Inclusive segmented scan over the lanes of a wave, distances 1, 2, ..., 32: afterwards the LAST lane of a run of equal `seg` holds the run's fold.
template <int N, typename T, typename Op> __device__ __forceinline__ void seg_scan(T (&v)[N], int seg, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool take = __shfl_up(seg, d, 64) == seg && lane >= d;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const T o = __shfl_up(v[i], d, 64);
            if (take) v[i] = Op::op(v[i], o);
        }
    }
}
__device__ __forceinline__ bool seg_last(int seg, int lane) { return __shfl_down(seg, 1, 64) != seg || lane == 63; }

// The segment of position p in a table of ascending offsets (cnt + 1 entries, positions counted from off[0]): the last one whose offset is <= p.
__device__ inline int64_t offsets_segment_at(const int64_t *__restrict__ off, int64_t cnt, int64_t p) {
    const int64_t v_lo = off[0];
    int64_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] - v_lo <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- the halo tile ---------------------------------------------------------------------------------------------------------------------
static constexpr int PK_C = 64, PK_R = 8, PK_S = 8;          // voxels of a tile: a wave reads one row of 64 along c (256 B)
static constexpr int PK_HC = PK_C + 2, PK_HR = PK_R + 2, PK_HS = PK_S + 2;
static constexpr int PK_THREADS = 256;

// Stage a tile of 64 x 8 x 8 voxels and its one-voxel halo: a wave per (s, r) row, 64 lanes along c (coalesced) and two lanes more for the far
// halo columns; five rows in flight per wave (the loads of a batch are issued before the first LDS store).  Outside the box: `outside`.
template <typename T>
__device__ __forceinline__ void halo_stage(T (*tile)[PK_HR][PK_HC], const T *__restrict__ src, int64_t pitch_c, int64_t pitch_r, int c0, int r0, int s0,
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

}  // namespace pdbeda
