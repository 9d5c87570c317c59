// tests/jobplan_harness.cpp -- the host's planner of labelling jobs and quanta (pdb_eda_amd/csrc/pdbeda_jobplan.h) as a stand-alone program.
//
// Test infrastructure (CPU): tests/test_jobplan_host.py writes cases into a text file, builds this file with the host compiler under
// AddressSanitizer + UBSan (float-cast-overflow included), runs it and compares what it prints with a restatement in Python integers.  Doubles
// travel as hexadecimal floats ("inf" and "nan" as those words).  One record a line:
//   tiles D0 D1 D2 TC TR TS             tile_grid                      -> "tiles NC NR NS N REFUSAL"
//   plan UC UR US PLANES WORST LABELS   plan_whole_map                 -> "plan" and every field of WholeMapPlan in the order of the struct
//   keys TOTAL_KEYS N_TILES             plan_key_table                 -> "keys" and every field of KeyTable in the order of the struct
//   shift BOUND                         quantum_shift                  -> "shift S"
//   mapq SUM_ABS MAX_ABS                map_quantum                    -> "mapq REFUSED MUL"
//   boxq MAX_ABS N_VOX                  box_quantum                    -> "boxq MUL"
//   coarse MUL LARGEST                  coarsened_for                  -> "coarse MUL"
//   model N_GRIDDED A_MAX               model_shift                    -> "model S"
// An accepted plan and every key table are also held to what the kernels and the host's casts rely on (check_*): a miss is reported on stderr and
// ends the program with status 3.
#include "pdbeda_jobplan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace pdbeda;

namespace {

long long integer(std::istream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "jobplan_harness: an integer is missing\n"); exit(2); }
    return v;
}
double real(std::istream &in) {
    std::string t;
    if (!(in >> t)) { fprintf(stderr, "jobplan_harness: a number is missing\n"); exit(2); }
    char *end = nullptr;
    const double v = strtod(t.c_str(), &end);
    if (end == t.c_str() || *end) { fprintf(stderr, "jobplan_harness: '%s' is no number\n", t.c_str()); exit(2); }
    return v;
}
void hold(bool ok, const char *what, const std::string &line) {
    if (!ok) { fprintf(stderr, "jobplan_harness: %s does not hold for '%s'\n", what, line.c_str()); exit(3); }
}

// What the kernels take for granted about a key table: the prefix table fits its LDS array, the counters come in whole groups, the tiles' clears
// cover the bitmap, the counters in use and the byte counters, and the group totals exist exactly where k_group_counts is launched.
void check_key_table(const KeyTable &k, int64_t n_tiles, const std::string &line) {
    hold(k.n_groups <= KEY_GROUPS, "n_groups <= KEY_GROUPS", line);
    hold(k.fine_shift >= 4 && k.fine_per_group == 1 << k.fine_shift, "fine_per_group is 2^fine_shift >= 16", line);
    hold(k.n_fine_alloc % k.fine_per_group == 0 && k.n_fine_alloc >= k.n_fine, "n_fine_alloc is whole groups that hold n_fine", line);
    hold((int64_t)k.n_groups * k.fine_per_group == k.n_fine_alloc, "n_groups groups are n_fine_alloc counters", line);
    hold((int64_t)k.key_bits_elems >= k.key_words && k.key_bits_elems % KEY_FINE == 0, "key_bits is whole buckets that hold key_words", line);
    hold((int64_t)k.fine_count_elems * 2 >= k.n_fine_alloc, "fine_count holds n_fine_alloc 16-bit counters", line);
    hold((int64_t)k.mid_count_elems * 4 * 4 >= k.key_words, "mid_count holds a byte per 4 key words", line);
    hold(k.has_group_count == (n_tiles != 0 && k.fine_shift > 4), "group_count exists iff tiles and shift > 4", line);
    if (n_tiles) {
        hold((int64_t)k.clear_bits * n_tiles >= k.key_words, "clear_bits x tiles covers key_words", line);
        hold((int64_t)k.clear_fine * n_tiles >= k.n_fine_alloc / 2, "clear_fine x tiles covers the counters' words", line);
        hold((int64_t)k.clear_mid * n_tiles >= (int64_t)k.mid_count_elems, "clear_mid x tiles covers mid_count", line);
    } else {
        hold(k.clear_bits == 0 && k.clear_fine == 0 && k.clear_mid == 0, "no tiles, no clears", line);
    }
}

// What whole_map_enqueue and job_carve cast: ids to uint32 (the kernels hold them in 31 bits), the blob table's rows to uint32.
void check_plan(const WholeMapPlan &p, int n_planes, const std::string &line) {
    const int64_t lim = 1ll << 31;
    hold(p.max_runs < lim && p.max_comps < lim && p.tile_runs < lim && p.tile_comps < lim, "run and component ids < 2^31", line);
    hold(p.tiles_pp < lim && p.keys_pp < lim && p.rtiles <= 65535 && p.stiles <= 65535, "tiles and keys of a plane < 2^31, a 3-D grid", line);
    hold(p.max_blobs >= 1 && p.max_blobs <= 0xffffffffll, "blob_cap <= 2^32 - 1 without the clamp", line);
    hold(p.cw >= 1 && p.cw <= 4 && (int64_t)p.ctiles * p.cw >= p.row_words && (int64_t)(p.ctiles - 1) * p.cw < p.row_words, "tiles of 1..4 words cover a row, none empty", line);
    hold(p.unit_ids >= 1 && p.unit_ids <= p.worst_unit && p.max_blobs <= p.worst_blobs, "the typical size is at most the worst case", line);
    hold(p.max_runs == p.tile_runs + p.unit_ids && p.max_comps == p.tile_comps + p.unit_ids, "unit ids above the tiles' ranges", line);
    hold(p.total_keys == p.keys_pp * n_planes && p.total_words == p.words_pp * n_planes, "planes", line);
    check_key_table(plan_key_table(p.total_keys, p.tiles_pp), p.tiles_pp, line);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: jobplan_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "jobplan_harness: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind) || kind[0] == '#') continue;
        if (kind == "tiles") {
            int d[3], t[3];
            for (int k = 0; k < 3; ++k) d[k] = (int)integer(in);
            for (int k = 0; k < 3; ++k) t[k] = (int)integer(in);
            const TileGrid g = tile_grid(d, t[0], t[1], t[2]);
            printf("tiles %d %d %d %lld %d\n", g.nc, g.nr, g.ns, (long long)g.n, g.refusal);
        } else if (kind == "plan") {
            const int uc = (int)integer(in), ur = (int)integer(in), us = (int)integer(in), n_planes = (int)integer(in);
            const bool worst = integer(in) != 0, labels = integer(in) != 0;
            const WholeMapPlan p = plan_whole_map(uc, ur, us, n_planes, worst, labels);
            printf("plan %d %d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %zu\n", p.refusal, p.row_words, p.ctiles, p.cw, p.rtiles,
                   p.stiles, (long long)p.tiles_pp, (long long)p.words_pp, (long long)p.keys_pp, (long long)p.total_words, (long long)p.total_keys,
                   (long long)p.worst_blobs, (long long)p.tile_runs, (long long)p.tile_comps, (long long)p.worst_unit, (long long)p.run_ids_needed,
                   (long long)p.unit_ids, (long long)p.max_runs, (long long)p.max_comps, (long long)p.max_blobs, p.lab_elems);
            if (p.refusal == PLAN_OK) check_plan(p, n_planes, line);
        } else if (kind == "keys") {
            const int64_t total_keys = integer(in), n_tiles = integer(in);
            const KeyTable k = plan_key_table(total_keys, n_tiles);
            printf("keys %lld %d %d %d %d %d %zu %zu %zu %d %d %d %d\n", (long long)k.key_words, k.n_fine, k.fine_shift, k.fine_per_group, k.n_groups, k.n_fine_alloc,
                   k.key_bits_elems, k.fine_count_elems, k.mid_count_elems, k.has_group_count ? 1 : 0, k.clear_bits, k.clear_fine, k.clear_mid);
            check_key_table(k, n_tiles, line);
        } else if (kind == "shift") {
            printf("shift %d\n", quantum_shift(real(in)));
        } else if (kind == "mapq") {
            const double sum_abs = real(in), max_abs = real(in);
            bool refused = false;
            const double mul = map_quantum(sum_abs, max_abs, &refused);
            printf("mapq %d %a\n", refused ? 1 : 0, mul);
        } else if (kind == "boxq") {
            const double max_abs = real(in);
            printf("boxq %a\n", box_quantum(max_abs, integer(in)));
        } else if (kind == "coarse") {
            const double mul = real(in);
            printf("coarse %a\n", coarsened_for(mul, integer(in)));
        } else if (kind == "model") {
            const int64_t n_gridded = integer(in);
            printf("model %d\n", model_shift(n_gridded, real(in)));
        } else {
            fprintf(stderr, "jobplan_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
