// pdbeda_jobplan.h -- the host's planner of labelling jobs and of every integer-sum quantum: a 3-D tile count with the limits of a launch, the
// whole-map job's tile grid, id ranges and arena sizes, the rank / key table of any job, and the rule that scales a sum so that it cannot leave
// 64 bits.  Plain integers and doubles only -- no HIP call, no pointer into device memory: the file compiles with the host compiler alone and
// runs under its sanitizers (tests/jobplan_harness.cpp); the callers are in pdbeda_hip.hip.  The constants the planner shares with the kernels
// are defined here, and the device headers include this file for them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace pdbeda {

constexpr int TILE_R = 8, TILE_S = 8;   // rows and sections of a whole-map tile (along c a tile is 1..4 mask words: TileDims::cw)
constexpr int TILE_COMPS = 256;   // component ids a whole-map tile owns (== CCAP of pdbeda_tile.h)
constexpr int KEY_FINE = 32;      // key words per fine counter (2048 keys)
constexpr int KEY_GROUPS = 1024;  // entries of the prefix table a k_emit block builds in LDS

// ---- A box in tiles -----------------------------------------------------------------------------------------------
// What may stand in a launch's way, as bits: a caller refuses on the ones its launch cares about, with its own message (a 1-D grid of tiles
// has no use for TILES_AXIS).
enum : int {
    TILES_EMPTY = 1,   // an axis without a voxel
    TILES_2P31 = 2,    // 2^31 tiles or more
    TILES_AXIS = 4     // more than 65 535 tiles along r or s (the y and z of a 3-D grid)
};
struct TileGrid {
    int nc, nr, ns;    // tiles along c, r, s
    int64_t n;         // their product
    int refusal;       // TILES_* bits, 0: none
};
static inline TileGrid tile_grid(const int dims[3], int tc, int tr, int ts) {
    TileGrid t;      // (the round-up in 64 bits: an axis of a stored grid may be within a tile edge of 2^31)
    t.nc = (int)(((int64_t)dims[0] + tc - 1) / tc);
    t.nr = (int)(((int64_t)dims[1] + tr - 1) / tr);
    t.ns = (int)(((int64_t)dims[2] + ts - 1) / ts);
    t.n = (int64_t)t.nc * t.nr * t.ns;
    t.refusal = ((dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) ? TILES_EMPTY : 0) | (t.n >= (1ll << 31) ? TILES_2P31 : 0) |
                ((t.nr > 65535 || t.ns > 65535) ? TILES_AXIS : 0);
    return t;
}

// ---- The whole-map job ----------------------------------------------------------------------------------------------
// Everything whole_map_enqueue derives from the unique box before it touches the device.  A job is enqueued for what maps need in practice --
// unit-tile run / component ids for a quarter of the tiles' own run-id range above the tiles' ranges, a blob table of one row per 32 keys --
// and, when that was too little, again for the worst case (worst_case: every other voxel a run of a unit tile, a blob per 2x2x2 cell).
enum : int {
    PLAN_OK = 0,
    PLAN_KEYS = 1,      // 2^31 tiles or keys in a plane, or more (first keys inside a plane are 31-bit)
    PLAN_AXIS = 2,      // more than 65 535 tiles along r or s (the tile kernels' grids are 3-D)
    PLAN_RUN_IDS = 3    // the tiles' run ids and the unit tiles' above them do not fit 31 bits: run_ids_needed
};
struct WholeMapPlan {
    int refusal;                                        // PLAN_*: the first that applies; what is derived behind that check stays 0
    int row_words, ctiles, cw, rtiles, stiles;          // mask words of a row; the tile grid; words of a tile along c
    int64_t tiles_pp, words_pp, keys_pp;                // per plane
    int64_t total_words, total_keys;
    int64_t worst_blobs, tile_runs, tile_comps, worst_unit;
    int64_t run_ids_needed;                             // tile_runs + worst_unit (what the PLAN_RUN_IDS message prints)
    int64_t unit_ids, max_runs, max_comps, max_blobs;
    size_t lab_elems;                                   // ONE signed label volume, also for a fused call
};
static inline WholeMapPlan plan_whole_map(int uc, int ur, int us, int n_planes, bool worst_case, bool labels) {
    WholeMapPlan p = WholeMapPlan();
    const int64_t half_c = ((int64_t)uc + 1) / 2, half_r = ((int64_t)ur + 1) / 2, half_s = ((int64_t)us + 1) / 2;      // (64 bits: an axis may be 2^31 - 1)
    p.row_words = (int)(((int64_t)uc + 63) / 64);
    p.words_pp = (int64_t)p.row_words * ur * us;
    p.keys_pp = (int64_t)uc * ur * us;
    p.total_words = p.words_pp * n_planes;
    p.total_keys = p.keys_pp * n_planes;
    // 26-connectivity: all voxels of an aligned 2x2x2 cell are mutually adjacent -> <= 1 blob per cell
    p.worst_blobs = half_c * half_r * half_s * n_planes + 1;
    p.lab_elems = labels ? (size_t)p.keys_pp : 0;
    const int words[3] = {p.row_words, ur, us};
    const TileGrid tg = tile_grid(words, 4, TILE_R, TILE_S);      // tiles of at most 4 mask words (256 voxels) along c ...
    p.ctiles = tg.nc; p.rtiles = tg.nr; p.stiles = tg.ns;
    p.cw = (p.row_words + p.ctiles - 1) / p.ctiles;               // ... of equal width: 5 words are 3 + 2, not 4 + 1
    p.tiles_pp = tg.n;
    if ((tg.refusal & TILES_2P31) || p.keys_pp >= (1ll << 31)) { p.refusal = PLAN_KEYS; return p; }
    if (tg.refusal & TILES_AXIS) { p.refusal = PLAN_AXIS; return p; }
    // run / component ids: a fixed range per tile (no allocation atomics) + the ids of the unit tiles above them
    p.tile_runs = p.tiles_pp * p.cw * 64 * 32;
    p.tile_comps = p.tiles_pp * TILE_COMPS;
    p.worst_unit = half_c * ur * us * n_planes + 1;       // every other voxel a run
    p.run_ids_needed = p.tile_runs + p.worst_unit;
    if (p.run_ids_needed >= (1ll << 31)) { p.refusal = PLAN_RUN_IDS; return p; }
    // (the typical size: a quarter of the tiles' own run-id range -- every tile a unit tile of 2 048 word-runs, or a quarter of them at the
    //  most a tile can hold: a protein-like map at 0.5 sigma, every tile over its LDS capacities, still runs once)
    p.unit_ids = worst_case ? p.worst_unit : std::min<int64_t>(p.worst_unit, std::max<int64_t>(65536, p.tile_runs / 4));
    p.max_blobs = worst_case ? p.worst_blobs : std::min<int64_t>(p.worst_blobs, std::max<int64_t>(4096, p.total_keys / 32));
    p.max_runs = p.tile_runs + p.unit_ids;
    p.max_comps = p.tile_comps + p.unit_ids;
    return p;
}

// ---- The rank / key table of a job ------------------------------------------------------------------------------------
// rank of a key = set bits of key_bits below it: one 16-bit counter per KEY_FINE key words (fine_count), a byte per 4 key words (mid_count), and
// the fine counters in groups of fine_per_group -- a power of two >= 16 that covers the job with KEY_GROUPS table entries.
struct KeyTable {
    int64_t key_words;
    int32_t n_fine, fine_shift, fine_per_group, n_groups, n_fine_alloc;
    size_t key_bits_elems;       // uint64: whole fine buckets (rank_of_key loads a bucket whole)
    size_t fine_count_elems;     // uint32: 16-bit counters, two per word, padded to whole groups
    size_t mid_count_elems;      // uint32: a byte per 4 key words, 8 per bucket
    bool has_group_count;        // groups of 32 counters or more in a whole-map job: maps beyond 2^25 keys = 256^3 fused
    int32_t clear_bits, clear_fine, clear_mid;      // words of each table a tile's k_face_merge workgroup clears (0 without tiles)
};
static inline KeyTable plan_key_table(int64_t total_keys, int64_t n_tiles) {
    KeyTable k = KeyTable();
    k.key_words = (total_keys + 63) / 64;
    const int64_t buckets = (k.key_words + KEY_FINE - 1) / KEY_FINE;
    k.n_fine = (int32_t)buckets;
    k.fine_shift = 4;
    while (((int64_t)KEY_GROUPS << k.fine_shift) < k.n_fine) k.fine_shift++;
    k.fine_per_group = 1 << k.fine_shift;
    k.n_groups = (k.n_fine + k.fine_per_group - 1) / k.fine_per_group;
    k.n_fine_alloc = (int32_t)((k.n_fine + k.fine_per_group - 1) / k.fine_per_group * k.fine_per_group);
    k.key_bits_elems = (size_t)buckets * KEY_FINE;
    k.fine_count_elems = (size_t)std::max(k.n_fine_alloc / 2, 8);
    k.mid_count_elems = (size_t)buckets * (KEY_FINE / 16);
    k.has_group_count = n_tiles && k.fine_shift > 4;
    if (n_tiles) {
        const int64_t nt = n_tiles, nfc = k.n_fine_alloc / 2, nmid = (int64_t)k.mid_count_elems;
        k.clear_bits = (int32_t)((k.key_words + nt - 1) / nt);
        k.clear_fine = (int32_t)((nfc + nt - 1) / nt);
        k.clear_mid = (int32_t)((nmid + nt - 1) / nt);
    }
    return k;
}

// ---- The quantum of the integer sums ------------------------------------------------------------------------------------
// A sum that decides something is kept in integers (FixSums in pdbeda_kernels.h): a term v enters as F = round(v * 2^S).  THE RULE: take a
// bound B on what the sum may reach, B < 2^e, and S = 61 - e: then B * 2^S < 2^61, at least 2^60 unless S was clamped, and the sum stays
// inside 64 bits with two bits to spare for the terms' roundings and their signs.  What follows from the bound each caller passes:
//   map_quantum   B = max(sum |rho|, 2^22 max |rho|) over the stored map.  sum |rho| * 2^S < 2^61: any set of stored voxels counted once -- a
//                 whole-map blob -- sums below 2^61.  max |rho| * 2^S < 2^39: a voxel's |F| < 2^39, so 2^22 voxels met in any way (a tile's or a
//                 run's first moment, a sphere's shell) sum below 2^61, and a batch that may meet a stored voxel again through the periodic
//                 wrap sums below 2^63 while it has fewer than 2^24 voxels (list_moments_compute refuses more).
//   box_quantum   B = max |rho| * max(voxels, 2^22) over a box: the same two bounds for sums over that box.
//   coarsened_for a sum over more than 2^22 voxels halves the quantum for every doubling beyond: voxels * max |F| stays below 2^61.
// S is 40 where the bound is zero, negative or not finite (nothing to scale by), and is kept inside [-900, 900] (ldexp(1.0, S) is a normal
// number; a map that clamps has voxels of 1e250 or of 1e-290 and was not measured).
static inline int quantum_shift(double bound) {
    int S = 40;
    if (bound > 0.0 && std::isfinite(bound)) {
        int e = 0;
        (void)frexp(bound, &e);        // bound < 2^e
        S = 61 - e;
    }
    return std::max(-900, std::min(S, 900));
}
// The integer sums cannot hold a NaN or an infinity (fix_of would saturate without a word): such a map is refused (*refused, 0.0 returned) by the
// labelling calls instead of producing wrong blob totals (the reference's sums would be NaN / inf for every blob that holds one).
static inline double map_quantum(double sum_abs, double max_abs, bool *refused) {
    *refused = !std::isfinite(sum_abs) || !std::isfinite(max_abs);
    if (*refused) return 0.0;
    return ldexp(1.0, quantum_shift(std::max(sum_abs, 4194304.0 * max_abs)));
}
// max_abs: the largest finite |rho| of the box (a float's magnitude: the product is finite).
static inline double box_quantum(double max_abs, int64_t n_vox) {
    return ldexp(1.0, quantum_shift(max_abs * (double)std::max<int64_t>(n_vox, 1ll << 22)));
}
static inline double coarsened_for(double fix_mul, int64_t largest /* voxels of the largest sum, < 2^62 */) {
    for (int64_t room = 1ll << 22; room < largest; room <<= 1) fix_mul *= 0.5;
    return fix_mul;
}
// The shift of the model density's integer sums: the largest S <= 40 with n_gridded * a_max * 2^S <= 2^62 (fp64; ldexp is exact).
static inline int model_shift(int64_t n_gridded, double a_max) {
    const double prod = (double)n_gridded * a_max;
    int S = 40;
    if (!(prod > 0.0)) return S;
    while (S > -1000 && ldexp(prod, S) > 0x1p62) --S;
    return S;
}

}  // namespace pdbeda
