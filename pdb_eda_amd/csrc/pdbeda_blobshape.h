// pdbeda_blobshape.h -- shape descriptors of the blobs of a list: bounding box, extreme voxel, geometric and |density|-weighted
// moments up to the second order.  No reference counterpart; the contract is spelled out at pdbeda_bloblist_moments in
// include/pdbeda.h.  Included from pdbeda_hip.hip.
//
// Input: the list's materialised voxel lists (crs grouped by blob + offsets, k_blob_offsets / k_voxel_lists).  The work is a segmented
// reduction over list POSITIONS: a workgroup of 256 takes BS_CHUNK consecutive positions whatever blobs they belong to, so one giant blob
// beside thousands of crumbs is spread like anything else.
//
//   k_blobshape_box      phase 1.  The blobs a chunk covers are consecutive; their offsets go to LDS (relative to the chunk) and every
//                        position finds its blob there.  Per voxel: the density (getPointDensityFromCrs: the one gather of the call),
//                        parked beside the blob index of the position for phase 2; per blob the maxima of (~c, ~r, ~s, c, r, s, bits of
//                        |rho|) -- the box and the largest |rho|, all as integer maxima.
//   k_blobshape_widths   the widest box of the list, for the host's check in front of phase 2 (offsets must stay below 2^15).
//   k_blobshape_sums     phase 2, relative to box_lo: the 9 integer sums, the 19 fixed-point ones (sum F, and F d / F d d' as two limbs,
//                        value = hi * 2^32 + lo, F = fix_of(|rho|): the FixSums idea of pdbeda_kernels.h) and, over the voxels whose |rho|
//                        IS the blob's maximum, the maximum of a key that orders them by offset, c most significant -- the tie rule.
//   k_blobshape_finish   integers -> the rows the host keeps with the list.
//
// Both phases reduce the same way (seg_fold): a segmented scan over the 64 positions of a wave (blob indices do not decrease along the
// lanes), then the last lane of every segment adds to the row of its blob in an LDS table of the chunk's first BS_SLOTS blobs, and the
// table goes to the per-blob records with one set of atomics per (workgroup, blob).  A blob beyond the table (a chunk of crumbs: more than
// BS_SLOTS blobs in BS_CHUNK voxels) gets the wave segment's atomics directly; a blob that spans chunks is the first blob of every chunk
// but the one it starts in, so the giant blob costs one set of atomics per workgroup.  Everything folded is an integer add or an integer
// maximum: no result depends on the order of the voxel list or of the atomics.
#pragma once
#include "pdbeda_kernels.h"
#include "pdbeda_wave.h"

namespace pdbeda {

static constexpr int BS_PER_THREAD = 8, BS_CHUNK = 256 * BS_PER_THREAD;      // list positions of a workgroup
static constexpr int BS_SLOTS = 128;                                         // blobs of a chunk that are summed in LDS
static constexpr int BS_BOX = 8;                                             // ints of a blob's box record: ~lo[3], hi[3], bits of max |rho|, -
static constexpr int BS_SUMS = 28, BS_REC = 32;                              // 64-bit words of a blob's sums record: the sums, the key, -
// the sums record: 0-2 sum d, 3-8 sum d d', 9 sum F, 10-15 (lo, hi) of sum F d, 16-27 (lo, hi) of sum F d d', 28 the extreme voxel's key
static constexpr int BS_KEY = 28;
static constexpr int BS_MAX_WIDTH = 1 << 15;

struct BlobShapeArgs {
    const Geom *geom;
    const float *dens;
    const int32_t *crs;             // the job's voxel lists
    const int64_t *off;             // offsets of the LIST's blobs into them: cnt + 1 entries
    int64_t cnt;                    // blobs of the list
    float *park_rho;                // per list position: the voxel's density ...
    int32_t *park_blob;             // ... and its blob (index in the list)
    int32_t *box;                   // [cnt][BS_BOX], starts as INT_MIN
    unsigned long long *rec;        // [cnt][BS_REC], starts as 0
    double fix_mul;
};

__global__ void __launch_bounds__(256) k_blobshape_box(BlobShapeArgs a) {
    __shared__ int s_off[BS_CHUNK + 1];
    __shared__ int s_box[BS_SLOTS * BS_BOX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t v_lo = a.off[0], nv = a.off[a.cnt] - v_lo;
    const int64_t chunk_lo = (int64_t)blockIdx.x * BS_CHUNK;
    if (chunk_lo >= nv) return;      // (block-uniform)
    const int n_here = (int)min((int64_t)BS_CHUNK, nv - chunk_lo);
    // every blob has a voxel, so the chunk covers at most n_here blobs
    const int64_t b_first = offsets_segment_at(a.off, a.cnt, chunk_lo), b_last = offsets_segment_at(a.off, a.cnt, chunk_lo + n_here - 1);
    const int nb_here = (int)(b_last - b_first + 1), n_slots = min(nb_here, BS_SLOTS);
    for (int i = tid; i <= nb_here; i += 256) {
        const int64_t rel = a.off[b_first + i] - v_lo - chunk_lo;      // (the first blob may start before the chunk, the last one end behind it)
        s_off[i] = (int)max((int64_t)0, min(rel, (int64_t)n_here));
    }
    for (int i = tid; i < n_slots * BS_BOX; i += 256) s_box[i] = INT_MIN;
    __syncthreads();
    const Geom &g = *a.geom;
    for (int k = 0; k < BS_PER_THREAD; ++k) {
        if (k * 256 + (tid & ~63) >= n_here) break;      // (wave-uniform: the shuffles below see whole waves)
        const int q = k * 256 + tid;
        int v[7] = {INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN};
        int lb = INT_MAX;      // (dead lanes: a segment of their own behind the live ones)
        if (q < n_here) {
            int lo = 0, hi = nb_here - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= q) lo = mid; else hi = mid - 1;
            }
            lb = lo;
            const int32_t *p = a.crs + 3 * (v_lo + chunk_lo + q);
            const int c = p[0], r = p[1], s = p[2];
            const float rho = fetch_wrapped(g, a.dens, c, r, s);
            a.park_rho[chunk_lo + q] = rho;
            a.park_blob[chunk_lo + q] = (int)(b_first + lb);
            v[0] = ~c; v[1] = ~r; v[2] = ~s; v[3] = c; v[4] = r; v[5] = s;
            v[6] = __float_as_int(fabsf(rho));      // (bits of a non-negative float: ordered like the integers)
        }
        seg_scan<7, int, SegMax>(v, lb, lane);
        if (seg_last(lb, lane) && lb != INT_MAX) {
            int *dst = lb < BS_SLOTS ? s_box + lb * BS_BOX : a.box + (b_first + lb) * BS_BOX;
#pragma unroll
            for (int i = 0; i < 7; ++i) atomicMax(dst + i, v[i]);
        }
    }
    __syncthreads();
    for (int i = tid; i < n_slots * BS_BOX; i += 256)
        if (s_box[i] != INT_MIN) atomicMax(a.box + b_first * BS_BOX + i, s_box[i]);
}

// *widest starts at 0.
__global__ void __launch_bounds__(256) k_blobshape_widths(const int32_t *__restrict__ box, int64_t cnt, unsigned long long *widest) {
    unsigned long long w = 0;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < cnt; b += (int64_t)gridDim.x * 256) {
        const int32_t *x = box + b * BS_BOX;
        for (int q = 0; q < 3; ++q) w = max(w, (unsigned long long)((long long)x[3 + q] - (long long)~x[q] + 1));
    }
    w = wave_fold<SegMax>(w);
    if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(widest, w);
}

__global__ void __launch_bounds__(256) k_blobshape_sums(BlobShapeArgs a) {
    __shared__ unsigned long long s_rec[BS_SLOTS * (BS_SUMS + 1)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t v_lo = a.off[0], nv = a.off[a.cnt] - v_lo;
    const int64_t chunk_lo = (int64_t)blockIdx.x * BS_CHUNK;
    if (chunk_lo >= nv) return;      // (block-uniform)
    const int n_here = (int)min((int64_t)BS_CHUNK, nv - chunk_lo);
    const int b_first = a.park_blob[chunk_lo], b_last = a.park_blob[chunk_lo + n_here - 1];
    const int n_slots = min(b_last - b_first + 1, BS_SLOTS);
    for (int i = tid; i < n_slots * (BS_SUMS + 1); i += 256) s_rec[i] = 0ull;
    __syncthreads();
    for (int k = 0; k < BS_PER_THREAD; ++k) {
        if (k * 256 + (tid & ~63) >= n_here) break;      // (wave-uniform)
        const int q = k * 256 + tid;
        unsigned long long v[BS_SUMS], key[1] = {0ull};
#pragma unroll
        for (int i = 0; i < BS_SUMS; ++i) v[i] = 0ull;
        int b = INT_MAX;
        if (q < n_here) {
            b = a.park_blob[chunk_lo + q];
            const float rho = a.park_rho[chunk_lo + q];
            const int32_t *p = a.crs + 3 * (v_lo + chunk_lo + q);
            const int32_t *x = a.box + (int64_t)b * BS_BOX;
            // offsets from the blob's own box: below 2^15 each (the host has checked the widths), so every product below is exact
            const unsigned long long d[3] = {(unsigned long long)((long long)p[0] - (long long)~x[0]), (unsigned long long)((long long)p[1] - (long long)~x[1]),
                                             (unsigned long long)((long long)p[2] - (long long)~x[2])};
            const unsigned long long F = (unsigned long long)fix_of((double)fabsf(rho), a.fix_mul);      // (< 2^39: map_fix_mul)
            v[0] = d[0]; v[1] = d[1]; v[2] = d[2];
            v[9] = F;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const unsigned long long Fd = F * d[i];      // (< 2^54)
                v[10 + 2 * i] = Fd & 0xffffffffull; v[11 + 2 * i] = Fd >> 32;
#pragma unroll
                for (int j = i; j < 3; ++j) {
                    const int t = 3 * i - i * (i - 1) / 2 + (j - i);      // cc cr cs rr rs ss
                    v[3 + t] = d[i] * d[j];
                    const unsigned __int128 Fdd = (unsigned __int128)Fd * d[j];      // (< 2^69: the high limb stays below 2^37)
                    v[16 + 2 * t] = (unsigned long long)(Fdd & 0xffffffffull); v[17 + 2 * t] = (unsigned long long)(Fdd >> 32);
                }
            }
            if (__float_as_int(fabsf(rho)) == x[6])      // a voxel with the blob's largest |rho|: the earlier in (c, r, s) order, the larger the key
                key[0] = (1ull << 62) - ((((d[0] << 30) | (d[1] << 15) | d[2]) << 1) | (unsigned long long)(__float_as_uint(rho) >> 31));
        }
        seg_scan<BS_SUMS, unsigned long long, SegAdd>(v, b, lane);
        seg_scan<1, unsigned long long, SegMax>(key, b, lane);
        if (seg_last(b, lane) && b != INT_MAX) {
            const int lb = b - b_first;
            if (lb < BS_SLOTS) {
                unsigned long long *dst = s_rec + lb * (BS_SUMS + 1);
#pragma unroll
                for (int i = 0; i < BS_SUMS; ++i)
                    if (v[i]) atomicAdd(dst + i, v[i]);
                if (key[0]) atomicMax(dst + BS_SUMS, key[0]);
            } else {
                unsigned long long *dst = a.rec + (int64_t)b * BS_REC;
#pragma unroll
                for (int i = 0; i < BS_SUMS; ++i)
                    if (v[i]) atomicAdd(dst + i, v[i]);
                if (key[0]) atomicMax(dst + BS_KEY, key[0]);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_slots * (BS_SUMS + 1); i += 256) {
        const int slot = i / (BS_SUMS + 1), f = i - slot * (BS_SUMS + 1);
        const unsigned long long t = s_rec[i];
        if (t == 0ull) continue;
        unsigned long long *dst = a.rec + (int64_t)(b_first + slot) * BS_REC + f;      // (f == BS_SUMS is the key's place, BS_KEY)
        if (f == BS_SUMS) atomicMax(dst, t); else atomicAdd(dst, t);
    }
}

// One thread per blob: the rows the host keeps.  out_i [cnt][10]: box_lo, box_hi, extreme crs, bits of the extreme value;
// out_l [cnt][9]: sum d, sum d d';  out_d [cnt][10]: sum w, sum w d, sum w d d' (one conversion each; fix_inv is a power of two).
__global__ void __launch_bounds__(256) k_blobshape_finish(const int32_t *__restrict__ box, const unsigned long long *__restrict__ rec, int64_t cnt, double fix_inv,
                                                          int32_t *__restrict__ out_i, long long *__restrict__ out_l, double *__restrict__ out_d) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= cnt) return;
    const int32_t *x = box + b * BS_BOX;
    const unsigned long long *r = rec + b * BS_REC;
    int32_t *oi = out_i + 10 * b;
    const int lo[3] = {~x[0], ~x[1], ~x[2]};
    const unsigned long long key = (1ull << 62) - r[BS_KEY], at = key >> 1;
    const int d[3] = {(int)(at >> 30), (int)((at >> 15) & 0x7fffull), (int)(at & 0x7fffull)};
    for (int q = 0; q < 3; ++q) { oi[q] = lo[q]; oi[3 + q] = x[3 + q]; oi[6 + q] = lo[q] + d[q]; }
    oi[9] = x[6] | (int)((unsigned)(key & 1ull) << 31);      // (|rho| with the voxel's sign bit)
    for (int i = 0; i < 9; ++i) out_l[9 * b + i] = (long long)r[i];
    double *od = out_d + 10 * b;
    od[0] = (double)(long long)r[9] * fix_inv;
    for (int i = 0; i < 9; ++i) od[1 + i] = fix_moment((long long)r[10 + 2 * i], (long long)r[11 + 2 * i]) * fix_inv;
}

}  // namespace pdbeda
