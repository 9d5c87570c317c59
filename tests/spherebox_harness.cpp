// tests/spherebox_harness.cpp -- the host's planner of sphere batches (pdb_eda_amd/csrc/pdbeda_spherebox.h) as a stand-alone program.
//
// Test infrastructure (CPU): tests/test_spherebox_host.py writes cases into a text file, builds this file with the host compiler under
// AddressSanitizer + UBSan (float-cast-overflow included), runs it and compares what it prints with a numpy restatement of the rule;
// tools/sanitize_cpu.sh runs the same.  Numbers are read with strtod (hex floats, nan, inf), one record a line:
//   geom  orthogonal map2xyz[3] map2crs[3] crs_start[3] xyz_interval[3] origin[3] grid_len[3] deortho[9]      the world of what follows
//   crs  x y z                        -> crs plannable c r s
//   halfwidths  r                     -> halfwidths plannable R0 R1 R2
//   spheres  n n_groups grouped       + n lines "x y z r group"
//                                     -> plan ..., "box" and "vol" lines when it fits, and for a per-atom batch the radii-only totals
//   bounds  n_groups n_boxes          + n_boxes lines "group_a group_b lo[3] hi[3]" (the box joins both groups; -1: none)
//                                     -> plan ..., "vol" lines when it fits
#include "pdbeda_spherebox.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

using namespace pdbeda;

namespace {

const int SMALL_ROWS = 512;      // (ATOM_WORDS of pdbeda_kernels.h, which only hipcc reads)

double num(std::istream &in) {
    std::string tok;
    if (!(in >> tok)) { fprintf(stderr, "spherebox_harness: a number is missing\n"); exit(2); }
    char *end = nullptr;
    const double v = strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) { fprintf(stderr, "spherebox_harness: bad number '%s'\n", tok.c_str()); exit(2); }
    return v;
}
long long integer(std::istream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "spherebox_harness: an integer is missing\n"); exit(2); }
    return v;
}

void print_plan(const SpherePlan &p) {
    printf("plan plannable %d fits %d", p.plannable ? 1 : 0, p.fits ? 1 : 0);
    if (p.fits) printf(" small_boxes %d words %lld keys %lld largest %lld", p.small_boxes ? 1 : 0, (long long)p.words, (long long)p.keys, (long long)p.largest);
    printf("\n");
}
void print_vols(const std::vector<VolDesc> &vols) {
    for (const VolDesc &v : vols)
        printf("vol %d %d %d %d %d %d %d %d %lld %lld\n", v.dim[0], v.dim[1], v.dim[2], v.org[0], v.org[1], v.org[2], v.row_words, v.group, (long long)v.word_base, (long long)v.key_base);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: spherebox_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "spherebox_harness: cannot read %s\n", argv[1]); return 2; }
    Geom g;
    memset(&g, 0, sizeof g);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind) || kind[0] == '#') continue;
        if (kind == "geom") {
            g.orthogonal = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.map2xyz[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.map2crs[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.crs_start[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.xyz_interval[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.origin[k] = num(in);
            for (int k = 0; k < 3; ++k) g.grid_len[k] = num(in);
            for (int k = 0; k < 9; ++k) g.deortho[k] = num(in);
        } else if (kind == "crs") {
            const double p[3] = {num(in), num(in), num(in)};
            int32_t c[3] = {0, 0, 0};
            const bool ok = plan_crs(g, p, c);
            printf("crs %d %d %d %d\n", ok ? 1 : 0, ok ? c[0] : 0, ok ? c[1] : 0, ok ? c[2] : 0);
        } else if (kind == "halfwidths") {
            const float r = (float)num(in);
            int32_t R[3] = {0, 0, 0};
            const bool ok = plan_half_widths(g, r, R);
            if (ok) {      // (the planner's half-widths ARE the rule's)
                int32_t S[3];
                sphere_half_widths(g, (double)r, S);
                if (memcmp(R, S, sizeof R) != 0) { fprintf(stderr, "spherebox_harness: plan_half_widths differs from sphere_half_widths\n"); return 1; }
            }
            printf("halfwidths %d %d %d %d\n", ok ? 1 : 0, ok ? R[0] : 0, ok ? R[1] : 0, ok ? R[2] : 0);
        } else if (kind == "spheres") {
            const long long n = integer(in), n_groups = integer(in), grouped = integer(in);
            std::vector<double> xyz(3 * (size_t)n);      // (exact sizes: a read or write past them is the sanitizer's to report)
            std::vector<float> radii((size_t)n);
            std::vector<int32_t> group((size_t)n);
            for (long long a = 0; a < n; ++a) {
                if (!std::getline(file, line)) { fprintf(stderr, "spherebox_harness: an atom is missing\n"); return 2; }
                std::istringstream at(line);
                for (int k = 0; k < 3; ++k) xyz[3 * (size_t)a + k] = num(at);
                radii[(size_t)a] = (float)num(at);
                group[(size_t)a] = (int32_t)integer(at);
            }
            std::vector<AtomBox> boxes((size_t)n);
            std::vector<VolDesc> vols((size_t)n_groups);
            const int32_t no_atom = 0;      // (an empty vector's data() may be null, and null says "a group per atom")
            const SpherePlan p = plan_spheres(g, xyz.data(), radii.data(), grouped ? (n ? group.data() : &no_atom) : nullptr, n, n_groups, boxes.data(), vols.data(), SMALL_ROWS);
            print_plan(p);
            if (p.fits) {
                for (const AtomBox &b : boxes) printf("box %d %d %d %d %d %d\n", b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
                print_vols(vols);
            }
            if (!grouped) {
                const SpherePlan r = plan_radii_totals(g, radii.data(), n, SMALL_ROWS);
                printf("radii ");
                print_plan(r);
            }
        } else if (kind == "bounds") {
            const long long n_groups = integer(in), n_boxes = integer(in);
            GroupBounds bounds(n_groups);
            for (long long b = 0; b < n_boxes; ++b) {
                if (!std::getline(file, line)) { fprintf(stderr, "spherebox_harness: a box is missing\n"); return 2; }
                std::istringstream bl(line);
                const long long ga = integer(bl), gb = integer(bl);
                AtomBox bx;
                for (int k = 0; k < 3; ++k) bx.lo[k] = (int32_t)integer(bl);
                for (int k = 0; k < 3; ++k) bx.hi[k] = (int32_t)integer(bl);
                if (ga >= 0) bounds.add(bx, ga);
                if (gb >= 0) bounds.add(bx, gb);
            }
            std::vector<VolDesc> vols((size_t)n_groups);
            SpherePlan plan{vols.data(), SMALL_ROWS};
            bounds.finish(plan);
            print_plan(plan);
            if (plan.fits) print_vols(vols);
        } else {
            fprintf(stderr, "spherebox_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
