// gradient_harness.cpp -- pdb_eda_amd/csrc/pdbeda_gradplan.h on a CPU: the header the library includes, compiled by the host compiler alone under
// AddressSanitizer + UBSan (tests/test_gradient_plan_host.py builds and runs it; nothing is loaded into Python).  One record per line of the cases file
// (numbers as strtod reads them: decimal, nan, inf):
//   check N NT FLAGS GIVEN  xyz[3 GIVEN] expo[GIVEN NT] radii[GIVEN]     -> check REFUSAL atom r_top       (GIVEN < N only where the count is refused first)
//   box rows[9] off[3] dom[3] x y z radius                              -> box lo_c lo_r lo_s n_c n_r n_s voxels clipped too_large
//   reach rows[9] r_max                                                 -> reach OK
//   shift max_w r_max v_max                                             -> shift S
// For every box the harness itself asserts what the kernel relies on (the box lies inside the domain, an empty box is all zeros); a miss, like a
// sanitizer report, ends it with a non-zero status.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pdbeda_gradplan.h"

using namespace pdbeda;

namespace {

void hold(bool ok, const char *what, const std::string &line) {
    if (ok) return;
    fprintf(stderr, "gradient_harness: %s does not hold for: %s\n", what, line.c_str());
    exit(1);
}

double number(std::istringstream &in) {
    std::string token;
    if (!(in >> token)) { fprintf(stderr, "gradient_harness: a number is missing\n"); exit(2); }
    char *end = nullptr;
    const double v = strtod(token.c_str(), &end);
    if (end == token.c_str() || *end) { fprintf(stderr, "gradient_harness: '%s' is no number\n", token.c_str()); exit(2); }
    return v;
}

long long integer(std::istringstream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "gradient_harness: an integer is missing\n"); exit(2); }
    return v;
}

void read_grid(std::istringstream &in, GradGrid *g, bool with_domain) {
    for (int i = 0; i < 9; ++i) g->rows[i] = number(in);
    if (with_domain) {
        for (int i = 0; i < 3; ++i) g->off[i] = number(in);
        for (int i = 0; i < 3; ++i) g->dom[i] = (int32_t)integer(in);
    }
    grad_grid_norms(g);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: gradient_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "gradient_harness: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "check") {
            const long long n = integer(in), nt = integer(in), flags = integer(in), given = integer(in);
            std::vector<double> xyz((size_t)(3 * given)), expo((size_t)(nt >= 1 && nt <= GP_MAX_TERMS ? given * nt : 0));      // (no exponents where n_terms is refused)
            std::vector<float> radii((size_t)given);
            for (double &v : xyz) v = number(in);
            for (double &v : expo) v = number(in);
            for (float &v : radii) v = (float)number(in);
            int64_t at = 0;
            float top = 0.0f;
            const int refusal = grad_check(xyz.data(), n, (int32_t)nt, expo.data(), radii.data(), (uint32_t)flags, 1u, &at, &top);
            hold(given == n || refusal == GRAD_TERMS || refusal == GRAD_FLAG || refusal == GRAD_COUNT, "arrays shorter than the count are never read", line);
            printf("check %d %lld %.17g\n", refusal, (long long)at, (double)top);
        } else if (kind == "box") {
            GradGrid g = GradGrid();
            read_grid(in, &g, true);
            double xyz[3];
            for (double &v : xyz) v = number(in);
            const double radius = number(in);
            GradBox b;
            bool clipped = false;
            const int64_t vox = grad_box(g, xyz, radius, &b, &clipped);
            for (int k = 0; k < 3; ++k) {
                if (vox == 0) hold(b.lo[k] == 0 && b.n[k] == 0, "an empty box is all zeros", line);
                else hold(b.lo[k] >= 0 && b.n[k] >= 1 && (int64_t)b.lo[k] + b.n[k] <= g.dom[k], "the box lies inside the domain", line);
            }
            hold(vox == (int64_t)b.n[0] * b.n[1] * b.n[2], "the voxels are the product of the sides", line);
            printf("box %d %d %d %d %d %d %lld %d %d\n", b.lo[0], b.lo[1], b.lo[2], b.n[0], b.n[1], b.n[2], (long long)vox, (int)clipped, (int)grad_box_too_large(vox));
        } else if (kind == "reach") {
            GradGrid g = GradGrid();
            read_grid(in, &g, false);
            printf("reach %d\n", (int)grad_reach_ok(g, number(in)));
        } else if (kind == "shift") {
            const double max_w = number(in), r_max = number(in);
            printf("shift %d\n", grad_shift(max_w, r_max, integer(in)));
        } else {
            fprintf(stderr, "gradient_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
