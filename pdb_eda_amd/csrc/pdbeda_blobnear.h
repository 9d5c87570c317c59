// pdbeda_blobnear.h -- nearest-blob search between two whole-map lists: for every blob of list a, the first entry of a caller-made
// offsets table that leads from one of its voxels into a blob of list b.  No reference counterpart; the contract is spelled out at
// pdbeda_bloblist_nearest in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
// Input: a's materialised voxel lists (crs grouped by blob + offsets, k_blob_offsets / k_voxel_lists), the signed label volume that holds
// b's blobs, and the table as packed words (one byte per component, biased by 128: why the components stay inside [-127, 127]).  The work
// is split over list POSITIONS as in pdbeda_blobshape.h: a workgroup of 256 takes a chunk of consecutive positions whatever blobs they belong
// to (256 per position of a thread: one on a short list, so that its walks run side by side in many workgroups, up to BN_CHUNK on a long
// one), and the blobs of the chunk are found from their offsets in LDS.
//
//   k_blobnear_scan     A LANE WALKS THE TABLE FOR ITS OWN VOXEL (the choice between the two forms the design left open; DESIGN.md 4.9 has
//                       the reasons).  The table is staged in LDS a piece of BN_PIECE entries at a time.  A voxel's answer is the first t
//                       whose target lies inside the non-repeating box and carries a label of b's sign; it is folded as the 64-bit key
//                       t << 40 | c-major position by an integer minimum: a segmented scan over the 64 positions of a wave, the last lane
//                       of a segment into an LDS table of the chunk's first BN_SLOTS blobs, and that table into the per-blob records with
//                       one atomic per (workgroup, blob).  A blob beyond the table (a chunk of crumbs) gets the wave segment's atomic
//                       directly.  A voxel scans only t up to its blob's best so far (the LDS row, else the record): a minimum does not
//                       depend on the order it is folded in, so pruning cannot change it.
//   k_blobnear_finish   one thread per blob: key -> t, voxel, partner voxel, and the partner's index out of b's labels.
#pragma once
#include <climits>

#include "pdbeda_device.h"
#include "pdbeda_wave.h"

namespace pdbeda {

static constexpr int BN_PER_THREAD = 8, BN_CHUNK = 256 * BN_PER_THREAD;      // the most list positions of a workgroup
static constexpr int BN_MIN_GROUPS = 512;                                    // a chunk grows beyond 256 positions only where that leaves this many workgroups
static constexpr int BN_UNROLL = 4;                                          // label reads in flight per lane
static constexpr int BN_SLOTS = 128;                                         // blobs of a chunk whose minimum is kept in LDS
static constexpr int BN_PIECE = 4096;                                        // table entries staged in LDS at a time
static constexpr int BN_MAX_OFFSETS = 16384, BN_MAX_COMPONENT = 127;
static constexpr int BN_POS_BITS = 40;                                       // key = t << 40 | c-major position (below 2^31: whole_map_enqueue)
static constexpr unsigned long long BN_NONE = ~0ull;                         // no pair: what the records start as
static constexpr int BN_REFRESH = 64;                                        // table entries between two looks at the blob's best so far

struct BlobNearArgs {
    const int32_t *crs;             // a's job: the voxel lists
    const int64_t *off;             // offsets of a's blobs into them: cnt + 1 entries
    int64_t cnt;                    // blobs of a
    const int32_t *labels;          // signed label volume [us][ur][uc] that holds b's blobs
    int32_t sign;                   // b's sign in it
    int32_t uc, ur, us;             // header.uniqueNcrs
    const uint32_t *table;          // n_off packed offsets: (dc + 128) | (dr + 128) << 8 | (ds + 128) << 16
    int32_t n_off;
    int32_t per_thread;             // list positions of a thread: 1, 2, 4 or BN_PER_THREAD (the chunk of a workgroup is 256 times that)
    unsigned long long *best;       // [cnt], starts as BN_NONE
};

__host__ __device__ inline uint32_t blobnear_pack(int dc, int dr, int ds) { return (uint32_t)(dc + 128) | ((uint32_t)(dr + 128) << 8) | ((uint32_t)(ds + 128) << 16); }

__device__ inline bool blobnear_member(int32_t lab, int sign) { return sign > 0 ? lab > 0 : lab < 0; }

// The end (exclusive) of what a voxel still has to scan when its blob's best key so far is `k`: entries up to AND INCLUDING that key's t
// (an equal t with an earlier position wins).
__device__ inline int blobnear_end(unsigned long long k, int n_off) { return k == BN_NONE ? n_off : min(n_off, (int)(k >> BN_POS_BITS) + 1); }

__global__ void __launch_bounds__(256) k_blobnear_scan(BlobNearArgs a) {
    __shared__ int s_off[BN_CHUNK + 1];
    __shared__ uint32_t s_tab[BN_PIECE];
    __shared__ unsigned long long s_best[BN_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t v_lo = a.off[0], nv = a.off[a.cnt] - v_lo;
    const int chunk = 256 * a.per_thread;      // (<= BN_CHUNK)
    const int64_t chunk_lo = (int64_t)blockIdx.x * chunk;
    if (chunk_lo >= nv) return;      // (block-uniform)
    const int n_here = (int)min((int64_t)chunk, nv - chunk_lo);
    // every blob has a voxel, so the chunk covers at most n_here blobs
    const int64_t b_first = offsets_segment_at(a.off, a.cnt, chunk_lo), b_last = offsets_segment_at(a.off, a.cnt, chunk_lo + n_here - 1);
    const int nb_here = (int)(b_last - b_first + 1), n_slots = min(nb_here, BN_SLOTS);
    for (int i = tid; i <= nb_here; i += 256) {
        const int64_t rel = a.off[b_first + i] - v_lo - chunk_lo;      // (the first blob may start before the chunk, the last one end behind it)
        s_off[i] = (int)max((int64_t)0, min(rel, (int64_t)n_here));
    }
    for (int i = tid; i < n_slots; i += 256) s_best[i] = BN_NONE;
    __syncthreads();
    const int uc = a.uc, ur = a.ur, us = a.us;
    unsigned done = 0u;      // bit k: position k of the thread has its answer, or nothing left to scan that could beat its blob's best
    for (int piece_lo = 0; piece_lo < a.n_off; piece_lo += BN_PIECE) {
        const int piece_hi = min(a.n_off, piece_lo + BN_PIECE);
        if (piece_lo > 0) __syncthreads();      // (everybody is done with the piece before)
        for (int i = tid; i < piece_hi - piece_lo; i += 256) s_tab[i] = a.table[piece_lo + i];
        __syncthreads();
        bool more = false;
        for (int k = 0; k < a.per_thread; ++k) {
            if (k * 256 + (tid & ~63) >= n_here) break;      // (wave-uniform: the shuffles below see whole waves)
            const int q = k * 256 + tid;
            unsigned long long key = BN_NONE;
            int lb = INT_MAX;      // the position's blob among the chunk's (dead lanes: a segment of their own behind the live ones)
            if (q < n_here) {
                int lo = 0, hi = nb_here - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_off[mid] <= q) lo = mid; else hi = mid - 1;
                }
                lb = lo;
            }
            if (lb != INT_MAX && !(done & (1u << k))) {
                const volatile unsigned long long *peek = lb < BN_SLOTS ? s_best + lb : a.best + (b_first + lb);
                // (the record too: workgroups that took other chunks of a large blob have left their minimum there)
                unsigned long long known = *peek;
                if (lb < BN_SLOTS) known = min(known, *(const volatile unsigned long long *)(a.best + (b_first + lb)));
                int limit = blobnear_end(known, a.n_off), t_end = min(piece_hi, limit);
                const int32_t *p = a.crs + 3 * (v_lo + chunk_lo + q);
                const int c = p[0], r = p[1], s = p[2];
                // BN_UNROLL entries a step: their label reads are issued together (the walk is a chain of read latencies otherwise)
                for (int t = piece_lo; t < t_end; t += BN_UNROLL) {
                    int32_t lab[BN_UNROLL];
#pragma unroll
                    for (int u = 0; u < BN_UNROLL; ++u) {
                        lab[u] = 0;      // (no blob of either sign)
                        if (t + u < t_end) {
                            const uint32_t w = s_tab[t + u - piece_lo];
                            const int c2 = c + (int)(w & 255u) - 128, r2 = r + (int)((w >> 8) & 255u) - 128, s2 = s + (int)((w >> 16) & 255u) - 128;
                            if ((unsigned)c2 < (unsigned)uc && (unsigned)r2 < (unsigned)ur && (unsigned)s2 < (unsigned)us)
                                lab[u] = a.labels[((int64_t)s2 * ur + r2) * uc + c2];
                        }
                    }
                    int hit = -1;
#pragma unroll
                    for (int u = BN_UNROLL - 1; u >= 0; --u)
                        if (blobnear_member(lab[u], a.sign)) hit = u;      // (the first of the step)
                    if (hit >= 0) {
                        key = ((unsigned long long)(t + hit) << BN_POS_BITS) | (unsigned long long)(((int64_t)c * ur + r) * us + s);
                        break;
                    }
                    if (((t - piece_lo) & (BN_REFRESH - 1)) == BN_REFRESH - BN_UNROLL) {
                        limit = min(limit, blobnear_end(*peek, a.n_off));
                        t_end = min(t_end, limit);
                    }
                }
                // done: an answer, or the blob's best ends inside this piece (or the table does)
                if (key != BN_NONE || limit <= piece_hi) done |= 1u << k;
                else more = true;
            }
            if (__any(key != BN_NONE)) {      // (wave-uniform)
                unsigned long long v[1] = {key};
                seg_scan<1, unsigned long long, SegMin>(v, lb, lane);
                if (seg_last(lb, lane) && lb != INT_MAX && v[0] != BN_NONE) atomicMin(lb < BN_SLOTS ? s_best + lb : a.best + (b_first + lb), v[0]);
            }
        }
        if (!__syncthreads_or(more ? 1 : 0)) break;      // (block-uniform)
    }
    __syncthreads();
    for (int i = tid; i < n_slots; i += 256)
        if (s_best[i] != BN_NONE) atomicMin(a.best + b_first + i, s_best[i]);
}

// One thread per blob of a.  out [cnt][8]: index, partner, voxel c r s, partner voxel c r s.
__global__ void __launch_bounds__(256) k_blobnear_finish(BlobNearArgs a, int32_t *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.cnt) return;
    int32_t *o = out + 8 * b;
    const unsigned long long key = a.best[b];
    if (key == BN_NONE) {
        o[0] = -1; o[1] = -1;
        for (int i = 2; i < 8; ++i) o[i] = 0;
        return;
    }
    const int t = (int)(key >> BN_POS_BITS);
    const int64_t pos = (int64_t)(key & ((1ull << BN_POS_BITS) - 1ull));
    const int s = (int)(pos % a.us), r = (int)((pos / a.us) % a.ur), c = (int)(pos / ((int64_t)a.us * a.ur));
    const uint32_t w = a.table[t];
    const int c2 = c + (int)(w & 255u) - 128, r2 = r + (int)((w >> 8) & 255u) - 128, s2 = s + (int)((w >> 16) & 255u) - 128;
    const int32_t lab = a.labels[((int64_t)s2 * a.ur + r2) * a.uc + c2];      // (inside the box and of b's sign: the scan has looked)
    o[0] = t; o[1] = a.sign > 0 ? lab - 1 : -lab - 1;
    o[2] = c; o[3] = r; o[4] = s; o[5] = c2; o[6] = r2; o[7] = s2;
}

}  // namespace pdbeda
