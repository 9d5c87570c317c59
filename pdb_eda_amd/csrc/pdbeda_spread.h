// pdbeda_spread.h -- the ordered spread of a mask: for every stored voxel the first entry of a caller-made offsets table that leads to a seed, and
// a value looked up by that rank.  No reference counterpart; the contract is spelled out at pdbeda_map_spread in include/pdbeda.h, the plan (the
// tile, the staged box, the row compilation of a table) in pdbeda_spreadplan.h.  Included from pdbeda_hip.hip.
//
//   k_spread<ROWS>   a workgroup of 256 owns a tile of SP_TILE_C x tile_r x tile_s outputs.  It stages the SEED BITS of the tile grown by the table's
//                    reach in LDS: a wave reads 64 consecutive voxels of a row through the wrap rule, compares them with the threshold, and the
//                    ballot is the 64-bit word (a staged row is one word without a reach along c, else two: bit 0 of the row is c0 - reach_c).
//                    A tile whose box holds no seed writes values[n] and is done.  Then a lane owns a voxel of a row of the tile, a wave a row:
//                    ROWS  the row records are read through uniform loads; per record the two staged words of the row (dr, ds) are shifted so
//                          that the lane's window starts at bit 0, one bit scan finds the first seed at or above the row's minimum and one the
//                          last seed below it, and two lookups in the uint16 rank array (in LDS behind the bits) give the candidates.  The wave
//                          leaves the loop at the first record whose best rank no lane can still use.
//                    walk  t = 0, 1, ... in lockstep, the packed offsets through uniform loads, one bit test each, until every lane has its seed.
//                    The value is values[t] (times base[v] in fp64, rounded once).
//                    Counters: every wave counts the seeds and the reached voxels of its rows by ballots; thread 0 writes the tile's two counts to
//                    the tile's own slot.
//   k_spread_fold    one workgroup: the slots into two int64 (integer sums: any order gives the same).
//
// A lane owns its voxel: no atomic, no reduction of values across lanes, nothing that depends on scheduling.
#pragma once
#include "pdbeda_device.h"
#include "pdbeda_spreadplan.h"

namespace pdbeda {

struct SpreadArgs {
    const float *x;                  // the map
    const float *base;               // null: the value itself
    float *out;
    int32_t nc, nr, ns;
    int32_t ic, ir, is;              // crs intervals
    float threshold;
    int32_t below;
    int32_t reach_c, reach_r, reach_s;
    int32_t tile_r, tile_s, words, box_r, box_s, n_words;
    int32_t tiles_c, tiles_r;
    const SpreadRow *rows;           // ROWS: n_rows records sorted by best, and the rank array
    int32_t n_rows;
    const uint16_t *ranks;
    int32_t n_ranks;
    const uint32_t *packed;          // walk: n_off packed offsets (spread_pack)
    int32_t n_off;
    const float *values;             // n_off + 1
    uint32_t *counts;                // [tiles][2]: seeds, reached
};

// Bits start .. start + 63 of the 128-bit row w1:w0 (zeros beyond it); start in 0 .. 127.
__device__ inline uint64_t spread_window(uint64_t w0, uint64_t w1, int start) {
    const uint64_t lo = start >= 64 ? w1 : w0, hi = start >= 64 ? 0ull : w1;
    const int sh = start & 63;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

template <bool ROWS>
__global__ void __launch_bounds__(256) k_spread(SpreadArgs a) {
    extern __shared__ uint64_t s_bits[];      // [box_s][box_r][words], then the ranks
    __shared__ uint32_t s_count[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t blk = blockIdx.x;
    const int c0 = (int)(blk % a.tiles_c) * SP_TILE_C;
    blk /= a.tiles_c;
    const int r0 = (int)(blk % a.tiles_r) * a.tile_r, s0 = (int)(blk / a.tiles_r) * a.tile_s;
    uint16_t *s_ranks = reinterpret_cast<uint16_t *>(s_bits + a.n_words);
    if (ROWS)
        for (int i = tid; i < a.n_ranks; i += 256) s_ranks[i] = a.ranks[i];
    // ---- the seed bits of the box
    bool any = false;
    for (int i = wave; i < a.n_words; i += 4) {      // (wave-uniform: the ballot sees whole waves)
        const int w = i % a.words, row = i / a.words;
        const int y = row % a.box_r, z = row / a.box_r;
        const int r = wrap_axis(r0 - a.reach_r + y, a.nr, a.ir), s = wrap_axis(s0 - a.reach_s + z, a.ns, a.is);
        const int c = wrap_axis(c0 - a.reach_c + 64 * w + lane, a.nc, a.ic);
        bool seed = false;
        if (r >= 0 && s >= 0 && c >= 0) {
            const float v = a.x[((int64_t)s * a.nr + r) * a.nc + c];
            seed = a.below ? v < a.threshold : v > a.threshold;      // (float32 against float32 is the comparison of the widened values; a NaN is neither)
        }
        const uint64_t word = __ballot(seed);
        if (lane == 0) s_bits[i] = word;
        any |= word != 0ull;
    }
    const bool some = __syncthreads_or(any ? 1 : 0) != 0;      // (also: the bits and the ranks are in place)
    // ---- the tile's outputs
    const int n_off = a.n_off;
    const int c = c0 + lane;
    uint32_t n_seed = 0u, n_reached = 0u;
    for (int q = wave; q < a.tile_r * a.tile_s; q += 4) {
        const int j = q % a.tile_r, k = q / a.tile_r;
        const int r = r0 + j, s = s0 + k;
        if (r >= a.nr || s >= a.ns) continue;      // (wave-uniform)
        const bool live = c < a.nc;
        int best = live ? n_off : -1;      // (a dead lane holds nobody up)
        if (some) {
            const int pos = lane + a.reach_c;      // the lane's own bit in a staged row
            if (ROWS) {
                for (int i = 0; i < a.n_rows; ++i) {
                    const SpreadRow rec = a.rows[i];
                    if (!__any(best > rec.best)) break;
                    const uint64_t *p = s_bits + ((k + a.reach_s + rec.ds) * a.box_r + (j + a.reach_r + rec.dr)) * a.words;
                    const uint64_t w0 = p[0], w1 = a.words > 1 ? p[1] : 0ull;
                    if ((w0 | w1) == 0ull) continue;      // (wave-uniform)
                    const int below_m = rec.m - rec.lo, from_m = rec.len - below_m;      // both 0 .. 64, from_m >= 1
                    const uint64_t up = spread_window(w0, w1, pos + rec.m) & bits_below(from_m);
                    if (up) best = min(best, (int)s_ranks[rec.start + below_m + ctz64(up)]);
                    const uint64_t down = spread_window(w0, w1, pos + rec.lo) & bits_below(below_m);
                    if (down) best = min(best, (int)s_ranks[rec.start + 63 - clz64(down)]);
                }
            } else {
                for (int t = 0; t < n_off; ++t) {
                    if (!__any(best == n_off)) break;
                    const uint32_t o = a.packed[t];
                    const int dc = (int)(o & 255u) - 128, dr = (int)((o >> 8) & 255u) - 128, ds = (int)((o >> 16) & 255u) - 128;
                    const int at = pos + dc;      // 0 .. 127
                    const uint64_t word = s_bits[((k + a.reach_s + ds) * a.box_r + (j + a.reach_r + dr)) * a.words + (at >> 6)];
                    if (best == n_off && ((word >> (at & 63)) & 1ull)) best = t;
                }
            }
        }
        const uint64_t own = s_bits[((k + a.reach_s) * a.box_r + (j + a.reach_r)) * a.words + ((lane + a.reach_c) >> 6)];
        n_seed += (uint32_t)popc64(__ballot(live && ((own >> ((lane + a.reach_c) & 63)) & 1ull)));
        n_reached += (uint32_t)popc64(__ballot(live && best < n_off));
        if (live) {
            const int64_t at = ((int64_t)s * a.nr + r) * a.nc + c;
            const float val = a.values[best];
            if (a.base) a.out[at] = (float)((double)a.base[at] * (double)val);
            else a.out[at] = val;
        }
    }
    if (lane == 0) { s_count[wave][0] = n_seed; s_count[wave][1] = n_reached; }
    __syncthreads();
    if (tid < 2) a.counts[2 * (int64_t)blockIdx.x + tid] = s_count[0][tid] + s_count[1][tid] + s_count[2][tid] + s_count[3][tid];
}

// One workgroup of 256.  out: the seeds and the reached voxels of all tiles.
__global__ void __launch_bounds__(256) k_spread_fold(const uint32_t *__restrict__ counts, int64_t n_tiles, int64_t *__restrict__ out) {
    __shared__ int64_t s_sum[256][2];
    int64_t acc[2] = {0, 0};
    for (int64_t i = threadIdx.x; i < n_tiles; i += 256) { acc[0] += counts[2 * i]; acc[1] += counts[2 * i + 1]; }
    s_sum[threadIdx.x][0] = acc[0]; s_sum[threadIdx.x][1] = acc[1];
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) { s_sum[threadIdx.x][0] += s_sum[threadIdx.x + step][0]; s_sum[threadIdx.x][1] += s_sum[threadIdx.x + step][1]; }
        __syncthreads();
    }
    if (threadIdx.x < 2) out[threadIdx.x] = s_sum[0][threadIdx.x];
}

}  // namespace pdbeda
