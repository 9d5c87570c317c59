// pdbeda_spreadplan.h -- the host's plan of pdbeda_map_spread: the argument checks, the tile and the staged box of seed bits for a table's
// reach, the LDS that costs, and the ROW COMPILATION of an ordered table.  Plain integers -- no HIP call, no pointer into device memory: the
// file compiles with the host compiler alone and runs under its sanitizers (tests/spread_harness.cpp); the caller is pdbeda_map_spread in
// pdbeda_hip.hip, and pdbeda_spread.h includes this file for the constants and the row record.  The contract: include/pdbeda.h.
//
// Rows.  The offsets are grouped by (dr, ds).  A row is ELIGIBLE iff its dc are distinct and form a contiguous run [lo, hi], the ranks along dc
// strictly fall to one minimum at dc = m and strictly rise behind it, and neither side of the minimum -- [lo, m - 1] and [m, hi] -- is longer
// than 64 offsets (the kernel looks at a side as ONE 64-bit window; only a row of all 65 offsets -32 .. 32 whose minimum sits on its first
// offset is lost to that).  A table is ROW-COMPILABLE iff it holds no duplicate offset and every row is eligible.  The smallest rank among
// the seeds of such a row is the smaller of two candidates: the first seed at or above m and the last one below m.  Records are sorted by
// `best`, the row's smallest rank, ascending: a voxel stops at the first record whose best is above what it has.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pdbeda {

constexpr int SP_MAX_OFFSETS = 16384;   // == PDBEDA_SPREAD_MAX_OFFSETS
constexpr int SP_MAX_REACH = 32;        // == PDBEDA_SPREAD_MAX_REACH: a staged row is at most two 64-bit words
constexpr int SP_TILE_C = 64;           // outputs of a tile along c: one lane each
constexpr int SP_TILE_R = 8;            // rows and sections of a tile where the staged box allows them (halved, s first, until it does)
constexpr int SP_TILE_S = 8;
constexpr int SP_LDS_TARGET = 40 * 1024;    // what a tile is shrunk for: four workgroups of a CU keep their boxes side by side
constexpr int SP_LDS_BUDGET = 128 * 1024;   // what the smallest tile may take at the largest reach and the longest table (it takes 100 368 B)

// What stands in the call's way, in the order the checks run (the first that applies).
enum : int {
    SPREAD_OK = 0,
    SPREAD_COUNT = 1,      // n_offsets outside 1 .. SP_MAX_OFFSETS
    SPREAD_REACH = 2,      // a component beyond +-SP_MAX_REACH
    SPREAD_THRESHOLD = 3,  // a NaN threshold
    SPREAD_FLAG = 4,       // an unknown flag
    SPREAD_AXIS = 5,       // an empty axis, an interval of 0, or an axis of 2^30 indices or more
    SPREAD_GRID = 6        // 2^31 tiles or more
};

// The checks that need no device.  offsets may be null only when n_offsets is refused first.  reach[3] gets max |dc|, |dr|, |ds|.
static inline int spread_check(const int32_t *offsets, int64_t n_offsets, bool threshold_nan, uint32_t flags, uint32_t known_flags, const int32_t ncrs[3],
                               const int32_t interval[3], int reach[3]) {
    reach[0] = reach[1] = reach[2] = 0;
    if (n_offsets < 1 || n_offsets > SP_MAX_OFFSETS) return SPREAD_COUNT;
    for (int64_t t = 0; t < n_offsets; ++t)
        for (int k = 0; k < 3; ++k) {
            const int32_t v = offsets[3 * t + k];
            if (v < -SP_MAX_REACH || v > SP_MAX_REACH) return SPREAD_REACH;
            reach[k] = std::max(reach[k], (int)(v < 0 ? -v : v));
        }
    if (threshold_nan) return SPREAD_THRESHOLD;
    if (flags & ~known_flags) return SPREAD_FLAG;
    for (int k = 0; k < 3; ++k)
        if (ncrs[k] <= 0 || ncrs[k] >= (1 << 30) || interval[k] <= 0) return SPREAD_AXIS;
    return SPREAD_OK;
}

// ---- The tile and its staged box ------------------------------------------------------------------------------------------------------
// A workgroup owns SP_TILE_C x tile_r x tile_s outputs and stages the seed bits of that box grown by the reach: box_r x box_s rows of `words`
// 64-bit words along c, the first bit at c0 - reach_c.  The uint16 ranks of a row-compiled table follow the words in LDS.
struct SpreadPlan {
    int refusal;                 // SPREAD_OK or SPREAD_GRID
    int tile_r, tile_s;
    int words;                   // of a staged row: 1 without a reach along c, else 2
    int box_r, box_s;            // staged rows and sections
    int n_words;                 // of the staged box
    int lds_bits, lds_ranks;     // bytes
    int lds_total;
    int tiles_c, tiles_r, tiles_s;
    int64_t n_tiles;
};
static inline int spread_lds_bits(const int reach[3], int tile_r, int tile_s) {
    const int words = reach[0] > 0 ? 2 : 1;
    return 8 * words * (tile_r + 2 * reach[1]) * (tile_s + 2 * reach[2]);
}
// n_ranks: the entries of the rank array (0 on the ordered walk, which keeps nothing but the bits in LDS).
static inline SpreadPlan plan_spread(const int32_t ncrs[3], const int reach[3], int n_ranks) {
    SpreadPlan p = SpreadPlan();
    p.lds_ranks = (2 * n_ranks + 7) / 8 * 8;
    p.tile_r = SP_TILE_R;
    p.tile_s = SP_TILE_S;
    while (spread_lds_bits(reach, p.tile_r, p.tile_s) + p.lds_ranks > SP_LDS_TARGET && (p.tile_r > 1 || p.tile_s > 1)) {
        if (p.tile_s >= p.tile_r) p.tile_s /= 2;
        else p.tile_r /= 2;
    }
    p.words = reach[0] > 0 ? 2 : 1;
    p.box_r = p.tile_r + 2 * reach[1];
    p.box_s = p.tile_s + 2 * reach[2];
    p.n_words = p.words * p.box_r * p.box_s;
    p.lds_bits = 8 * p.n_words;
    p.lds_total = p.lds_bits + p.lds_ranks;
    p.tiles_c = (int)(((int64_t)ncrs[0] + SP_TILE_C - 1) / SP_TILE_C);
    p.tiles_r = (int)(((int64_t)ncrs[1] + p.tile_r - 1) / p.tile_r);
    p.tiles_s = (int)(((int64_t)ncrs[2] + p.tile_s - 1) / p.tile_s);
    p.n_tiles = (int64_t)p.tiles_c * p.tiles_r * p.tiles_s;
    p.refusal = p.n_tiles >= (1ll << 31) ? SPREAD_GRID : SPREAD_OK;
    return p;
}

// ---- Row compilation ----------------------------------------------------------------------------------------------------------------------
struct SpreadRow {
    int32_t dr, ds;
    int32_t lo, len;     // the row's dc are lo .. lo + len - 1
    int32_t m;           // the dc of the row's smallest rank
    int32_t best;        // that rank
    int32_t start;       // of the row's len ranks (in ascending dc) in the rank array
    int32_t pad;
};

// true: rows (sorted by best) and ranks (n_offsets entries) describe the table.  false: the table is not row-compilable; both are left empty.
static inline bool spread_compile_rows(const int32_t *offsets, int64_t n_offsets, std::vector<SpreadRow> *rows, std::vector<uint16_t> *ranks) {
    rows->clear();
    ranks->clear();
    struct Entry { int32_t ds, dr, dc, t; };
    std::vector<Entry> e((size_t)n_offsets);
    for (int64_t t = 0; t < n_offsets; ++t) e[(size_t)t] = Entry{offsets[3 * t + 2], offsets[3 * t + 1], offsets[3 * t], (int32_t)t};
    std::sort(e.begin(), e.end(), [](const Entry &a, const Entry &b) {
        if (a.ds != b.ds) return a.ds < b.ds;
        if (a.dr != b.dr) return a.dr < b.dr;
        if (a.dc != b.dc) return a.dc < b.dc;
        return a.t < b.t;
    });
    struct Span { size_t first; SpreadRow row; };
    std::vector<Span> spans;
    for (size_t i = 0; i < e.size();) {
        size_t j = i + 1;
        while (j < e.size() && e[j].ds == e[i].ds && e[j].dr == e[i].dr) ++j;
        size_t at = i;      // the row's minimum
        for (size_t k = i + 1; k < j; ++k) {
            if (e[k].dc != e[k - 1].dc + 1) return false;      // a duplicate (the same dc again) or a gap
            if (e[k].t < e[at].t) at = k;
        }
        for (size_t k = i + 1; k < j; ++k)
            if (k <= at ? !(e[k].t < e[k - 1].t) : !(e[k].t > e[k - 1].t)) return false;
        if (at - i > 64 || j - at > 64) return false;
        SpreadRow r = SpreadRow();
        r.dr = e[i].dr; r.ds = e[i].ds;
        r.lo = e[i].dc; r.len = (int32_t)(j - i);
        r.m = e[at].dc; r.best = e[at].t;
        spans.push_back(Span{i, r});
        i = j;
    }
    std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.row.best < b.row.best; });
    ranks->reserve((size_t)n_offsets);
    for (Span &s : spans) {
        s.row.start = (int32_t)ranks->size();
        for (int32_t k = 0; k < s.row.len; ++k) ranks->push_back((uint16_t)e[s.first + (size_t)k].t);
        rows->push_back(s.row);
    }
    return true;
}

// The packed offset of the ordered walk: one byte per component, biased by 128.
static inline uint32_t spread_pack(int dc, int dr, int ds) { return (uint32_t)(dc + 128) | ((uint32_t)(dr + 128) << 8) | ((uint32_t)(ds + 128) << 16); }

}  // namespace pdbeda
