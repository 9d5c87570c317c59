// pose_harness.cpp -- pdb_eda_amd/csrc/pdbeda_poseplan.h on a CPU: the header the library includes, compiled by the host compiler alone under
// AddressSanitizer + UBSan (tests/test_pose_plan_host.py builds and runs it; nothing is loaded into Python).  One record per line of the cases file
// (numbers as strtod reads them: decimal, nan, inf):
//   check NF NR NC TOPK FLAGS GF GR GC  frag[3 GF] w[GF] rot[9 GR] centres[3 GC]   -> check REFUSAL offender radius   (G* < N* only where a count is refused first)
//   box rows[9] off[3] x y z radius GLOBAL_ONLY                                     -> box lo_c lo_r lo_s n_c n_r n_s voxels staged
//   centre rows[9] off[3] x y z                                                     -> centre OK
//   reach rows[9] radius                                                            -> reach OK
//   chunk NC NR                                                                     -> chunk CENTRES
//   scratch NF NR CHUNK TOPK                                                        -> scratch BYTES
// For every box, chunk and carve the harness itself asserts what the library relies on; a miss, like a sanitizer report, ends it with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pdbeda_poseplan.h"

using namespace pdbeda;

namespace {

void hold(bool ok, const char *what, const std::string &line) {
    if (ok) return;
    fprintf(stderr, "pose_harness: %s does not hold for: %s\n", what, line.c_str());
    exit(1);
}

double number(std::istringstream &in) {
    std::string token;
    if (!(in >> token)) { fprintf(stderr, "pose_harness: a number is missing\n"); exit(2); }
    char *end = nullptr;
    const double v = strtod(token.c_str(), &end);
    if (end == token.c_str() || *end) { fprintf(stderr, "pose_harness: '%s' is no number\n", token.c_str()); exit(2); }
    return v;
}

long long integer(std::istringstream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "pose_harness: an integer is missing\n"); exit(2); }
    return v;
}

void read_grid(std::istringstream &in, GradGrid *g, bool with_offset) {
    for (int i = 0; i < 9; ++i) g->rows[i] = number(in);
    if (with_offset)
        for (int i = 0; i < 3; ++i) g->off[i] = number(in);
    grad_grid_norms(g);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: pose_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "pose_harness: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "check") {
            const long long nf = integer(in), nr = integer(in), nc = integer(in), top_k = integer(in), flags = integer(in);
            const long long gf = integer(in), gr = integer(in), gc = integer(in);
            std::vector<double> frag((size_t)(3 * gf)), w((size_t)gf), rot((size_t)(9 * gr)), centres((size_t)(3 * gc));      // (exact sizes: ASan sees a read past what was given)
            for (double &v : frag) v = number(in);
            for (double &v : w) v = number(in);
            for (double &v : rot) v = number(in);
            for (double &v : centres) v = number(in);
            int64_t at = 0;
            double radius = -1.0;
            const int refusal = pose_check(frag.data(), w.data(), (int32_t)nf, rot.data(), nr, centres.data(), nc, (int32_t)top_k, (uint32_t)flags, 3u, &at, &radius);
            hold((gf == nf && gr == nr && gc == nc) || (refusal >= POSE_ATOMS && refusal <= POSE_COUNT), "arrays shorter than the counts are never read", line);
            printf("check %d %lld %.17g\n", refusal, (long long)at, radius);
        } else if (kind == "box") {
            GradGrid g = GradGrid();
            read_grid(in, &g, true);
            double c[3];
            for (double &v : c) v = number(in);
            const double radius = number(in);
            const bool global_only = integer(in) != 0;
            hold(pose_centre_ok(g, c) && grad_reach_ok(g, radius), "the box is asked for after the two checks", line);
            PoseBox b;
            const int64_t vox = pose_box(g, c, radius, global_only, &b);
            for (int k = 0; k < 3; ++k) hold(b.n[k] >= 2 * POSE_GROW, "a side holds the two corners and a voxel of safety on either side", line);      // (a pivot between voxels and no radius: an empty range)
            if (b.staged) {
                hold(!global_only && vox == (int64_t)b.n[0] * b.n[1] * b.n[2], "a staged box has its product", line);
                hold(pose_lds_bytes(vox) <= POSE_LDS_BUDGET && POSE_LDS_BUDGET <= 160 * 1024, "a staged box fits the budget, the budget a CU", line);
            } else {
                hold(global_only || vox < 0 || pose_lds_bytes(vox) > POSE_LDS_BUDGET, "a box within the budget is staged", line);
            }
            printf("box %d %d %d %d %d %d %lld %d\n", b.lo[0], b.lo[1], b.lo[2], b.n[0], b.n[1], b.n[2], (long long)vox, b.staged);
        } else if (kind == "centre") {
            GradGrid g = GradGrid();
            read_grid(in, &g, true);
            double c[3];
            for (double &v : c) v = number(in);
            printf("centre %d\n", (int)pose_centre_ok(g, c));
        } else if (kind == "reach") {
            GradGrid g = GradGrid();
            read_grid(in, &g, false);
            printf("reach %d\n", (int)grad_reach_ok(g, number(in)));
        } else if (kind == "chunk") {
            const long long nc = integer(in), nr = integer(in);
            const int64_t ch = pose_chunk(nc, nr);
            hold(ch >= 1 && ch <= std::max<long long>(nc, 1), "a chunk holds one centre at the least and no more than there are", line);
            hold(ch == 1 || ch * nr * POSE_TABLE_ROW <= POSE_TABLE_BYTES, "a chunk of several centres keeps the table within its limit", line);
            printf("chunk %lld\n", (long long)ch);
        } else if (kind == "scratch") {
            const long long nf = integer(in), nr = integer(in), ch = integer(in), top_k = integer(in);
            const size_t bytes = pose_scratch_bytes((int32_t)nf, nr, ch, (int32_t)top_k);
            std::vector<char> arena(bytes);      // the second pass of the carve, on a real base: every piece lies inside, in order, 256-byte aligned
            Carver cv(arena.data());
            PoseScratch s;
            s.carve(cv, (int32_t)nf, nr, ch, (int32_t)top_k);
            hold(cv.off == bytes, "the two passes of the carve end at one offset", line);
            hold((char *)s.frag == arena.data() && (char *)s.n_kept + 4 * ch <= arena.data() + bytes, "the pieces lie inside the arena", line);
            hold((char *)s.score >= (char *)(s.box + ch) && (char *)s.low >= (char *)(s.score + ch * nr) && (char *)s.kept >= (char *)(s.low + ch * nr), "the table's pieces do not overlap", line);
            printf("scratch %zu\n", bytes);
        } else {
            fprintf(stderr, "pose_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
