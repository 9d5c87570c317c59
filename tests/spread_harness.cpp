// spread_harness.cpp -- pdb_eda_amd/csrc/pdbeda_spreadplan.h on a CPU: the header the library includes, compiled by the host compiler alone under
// AddressSanitizer + UBSan (tests/test_spread_plan_host.py builds and runs it; nothing is loaded into Python).  One record per line of the cases file:
//   check N FLAGS NAN nc nr ns ic ir is  o...    -> check REFUSAL reach_c reach_r reach_s
//   plan nc nr ns reach_c reach_r reach_s RANKS  -> plan refusal tile_r tile_s words box_r box_s n_words lds_bits lds_ranks lds_total tiles_c tiles_r tiles_s n_tiles
//   rows N  o...                                 -> rows OK n_rows, then per record: row dr ds lo len m best start, then: ranks r...
// For every accepted plan and every compiled table the harness itself asserts what the kernel relies on (the box covers the tile grown by the reach,
// the LDS stays inside the budget, the records tile the rank array, and -- on pseudo-random seed words -- the two candidates of a row give the row's
// smallest seeded rank); a miss, like a sanitizer report, ends it with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "pdbeda_spreadplan.h"

using namespace pdbeda;

namespace {

void hold(bool ok, const char *what, const std::string &line) {
    if (ok) return;
    fprintf(stderr, "spread_harness: %s does not hold for: %s\n", what, line.c_str());
    exit(1);
}

long long integer(std::istringstream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "spread_harness: a number is missing\n"); exit(2); }
    return v;
}

uint64_t next_random(uint64_t *state) {      // (xorshift64)
    uint64_t x = *state;
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return *state = x;
}

// The kernel's two candidates of a row for a lane at bit `pos` of the 128-bit staged row w1:w0, restated with single-bit tests.
int two_candidates(const SpreadRow &r, const std::vector<uint16_t> &ranks, uint64_t w0, uint64_t w1, int pos, int none) {
    auto bit = [&](int at) { return at < 64 ? (w0 >> at) & 1u : (w1 >> (at - 64)) & 1u; };
    int best = none;
    for (int dc = r.m; dc < r.lo + r.len; ++dc)
        if (bit(pos + dc)) { best = std::min(best, (int)ranks[(size_t)(r.start + dc - r.lo)]); break; }
    for (int dc = r.m - 1; dc >= r.lo; --dc)
        if (bit(pos + dc)) { best = std::min(best, (int)ranks[(size_t)(r.start + dc - r.lo)]); break; }
    return best;
}

void check_rows(const std::vector<int32_t> &o, const std::vector<SpreadRow> &rows, const std::vector<uint16_t> &ranks, const std::string &line) {
    const int n = (int)(o.size() / 3);
    hold((int)ranks.size() == n, "one rank per offset", line);
    int at = 0, reach_c = 0;
    for (int t = 0; t < n; ++t) reach_c = std::max(reach_c, std::abs(o[3 * (size_t)t]));
    uint64_t state = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < rows.size(); ++i) {
        const SpreadRow &r = rows[i];
        hold(r.start == at && r.len >= 1, "the records tile the rank array", line);
        at += r.len;
        hold(i == 0 || rows[i - 1].best < r.best, "records in ascending best", line);
        hold(r.m >= r.lo && r.m < r.lo + r.len && r.m - r.lo <= 64 && r.lo + r.len - r.m <= 64, "a side of the minimum is one window", line);
        hold(ranks[(size_t)(r.start + r.m - r.lo)] == r.best, "best is the rank at m", line);
        for (int k = 0; k < r.len; ++k) {
            const int t = ranks[(size_t)(r.start + k)];
            hold(t < n && o[3 * (size_t)t] == r.lo + k && o[3 * (size_t)t + 1] == r.dr && o[3 * (size_t)t + 2] == r.ds, "a rank names its offset", line);
        }
        for (int trial = 0; trial < 8; ++trial) {
            uint64_t w0 = next_random(&state) & next_random(&state), w1 = next_random(&state) & next_random(&state);
            if (trial == 0) w0 = w1 = 0;
            if (trial == 1) w0 = w1 = ~0ull;
            const int pos = (int)(next_random(&state) % 64) + reach_c;
            int want = n;
            for (int k = 0; k < r.len; ++k) {
                const int b = pos + r.lo + k;
                if (b < 64 ? (w0 >> b) & 1u : (w1 >> (b - 64)) & 1u) want = std::min(want, (int)ranks[(size_t)(r.start + k)]);
            }
            hold(two_candidates(r, ranks, w0, w1, pos, n) == want, "two candidates give the row's smallest seeded rank", line);
        }
    }
    hold(at == n, "every offset is in a row", line);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: spread_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "spread_harness: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind) || kind[0] == '#') continue;
        if (kind == "check") {
            const long long n = integer(in);
            const uint32_t flags = (uint32_t)integer(in);
            const bool nan = integer(in) != 0;
            int32_t ncrs[3], interval[3];
            for (int k = 0; k < 3; ++k) ncrs[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) interval[k] = (int32_t)integer(in);
            std::vector<int32_t> o;
            long long v;
            while (in >> v) o.push_back((int32_t)v);
            hold(n < 1 || n > SP_MAX_OFFSETS || (long long)o.size() == 3 * n, "the record carries its offsets", line);
            int reach[3];
            const int refusal = spread_check(o.data(), n, nan, flags, 1u, ncrs, interval, reach);
            printf("check %d %d %d %d\n", refusal, reach[0], reach[1], reach[2]);
        } else if (kind == "plan") {
            int32_t ncrs[3];
            int reach[3];
            for (int k = 0; k < 3; ++k) ncrs[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) reach[k] = (int)integer(in);
            const int n_ranks = (int)integer(in);
            const SpreadPlan p = plan_spread(ncrs, reach, n_ranks);
            printf("plan %d %d %d %d %d %d %d %d %d %d %d %d %d %lld\n", p.refusal, p.tile_r, p.tile_s, p.words, p.box_r, p.box_s, p.n_words, p.lds_bits, p.lds_ranks, p.lds_total,
                   p.tiles_c, p.tiles_r, p.tiles_s, (long long)p.n_tiles);
            hold(p.tile_r >= 1 && p.tile_s >= 1 && p.box_r == p.tile_r + 2 * reach[1] && p.box_s == p.tile_s + 2 * reach[2], "the box is the tile grown by the reach", line);
            hold(64 * p.words >= SP_TILE_C + 2 * reach[0], "the words of a row hold the tile grown along c (the last bit a lane reads is 63 + 2 reach)", line);
            hold(p.lds_total <= SP_LDS_BUDGET && p.lds_ranks >= 2 * n_ranks && p.lds_bits % 8 == 0, "the LDS stays inside the budget", line);
            hold(p.lds_total <= SP_LDS_TARGET || (p.tile_r == 1 && p.tile_s == 1), "a tile is shrunk until it meets the target or is one row", line);
            if (p.refusal == SPREAD_OK)
                hold((int64_t)p.tiles_c * SP_TILE_C >= ncrs[0] && (int64_t)p.tiles_r * p.tile_r >= ncrs[1] && (int64_t)p.tiles_s * p.tile_s >= ncrs[2] && p.n_tiles < (1ll << 31),
                     "the tiles cover the map", line);
        } else if (kind == "rows") {
            const long long n = integer(in);
            std::vector<int32_t> o;
            long long v;
            while (in >> v) o.push_back((int32_t)v);
            hold((long long)o.size() == 3 * n, "the record carries its offsets", line);
            std::vector<SpreadRow> rows;
            std::vector<uint16_t> ranks;
            const bool ok = spread_compile_rows(o.data(), n, &rows, &ranks);
            printf("rows %d %zu\n", ok ? 1 : 0, rows.size());
            if (ok) check_rows(o, rows, ranks, line);
            else hold(rows.empty() && ranks.empty(), "a refused table leaves nothing", line);
            for (const SpreadRow &r : rows) printf("row %d %d %d %d %d %d %d\n", r.dr, r.ds, r.lo, r.len, r.m, r.best, r.start);
            printf("ranks");
            for (uint16_t r : ranks) printf(" %d", (int)r);
            printf("\n");
        } else {
            fprintf(stderr, "spread_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
