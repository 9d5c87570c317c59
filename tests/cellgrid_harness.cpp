// tests/cellgrid_harness.cpp -- the host's planner of cell grids (pdb_eda_amd/csrc/pdbeda_cellgrid.h) as a stand-alone program.
//
// Test infrastructure (CPU): tests/test_cellgrid_host.py writes cases into a text file, builds this file with the host compiler under
// AddressSanitizer + UBSan (float-cast-overflow included), runs it and compares what it prints with a Python restatement of the planner.
// Numbers are read with strtod (hex floats, inf); a double is printed as the 16 hex digits of its bit pattern.  One record a line:
//   geom  orthogonal map2xyz[3] crs_start[3] xyz_interval[3] origin[3] grid_len[3] ortho[9] deortho[9]      the world of what follows
//   grid  lo[3] hi[3] cutoff n_points                -> grid ... (make_cell_grid, the box its own crop box), or "refused axis"
//   query  n cutoff n_points   + n lines "x y z"     -> grid ... (query_grid), or "refused axis"
//   crop  blo[3] bhi[3] reach n   + n lines "x y z"  -> grid ... (crop_cell_grid), then "held" and the cell of every atom (-1: cropped)
//   corners  c0[3] c1[3]                             -> corners lo[3] hi[3] (crs_box_xyz)
//   reach  r                                         -> reach 0|1 (reach_below_2p29_steps)
#include "pdbeda_cellgrid.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace pdbeda;

namespace {

double num(std::istream &in) {
    std::string tok;
    if (!(in >> tok)) { fprintf(stderr, "cellgrid_harness: a number is missing\n"); exit(2); }
    char *end = nullptr;
    const double v = strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end) { fprintf(stderr, "cellgrid_harness: bad number '%s'\n", tok.c_str()); exit(2); }
    return v;
}
long long integer(std::istream &in) {
    long long v = 0;
    if (!(in >> v)) { fprintf(stderr, "cellgrid_harness: an integer is missing\n"); exit(2); }
    return v;
}
void num3(std::istream &in, double v[3]) { for (int k = 0; k < 3; ++k) v[k] = num(in); }

void print_bits(const double *v, int n) {
    for (int k = 0; k < n; ++k) {
        unsigned long long b;
        memcpy(&b, &v[k], 8);
        printf(" %016llx", b);
    }
}
void print_grid(const CellGrid &g) {
    printf("grid");
    print_bits(g.lo, 3);
    print_bits(&g.edge, 1);
    print_bits(g.crop_lo, 3);
    print_bits(g.crop_hi, 3);
    printf(" %d %d %d %d\n", g.dim[0], g.dim[1], g.dim[2], g.n_cells);
}
// (exact sizes: a read past them is the sanitizer's to report)
std::vector<double> points(std::ifstream &file, long long n) {
    std::vector<double> xyz(3 * (size_t)n);
    std::string line;
    for (long long i = 0; i < n; ++i) {
        if (!std::getline(file, line)) { fprintf(stderr, "cellgrid_harness: a point is missing\n"); exit(2); }
        std::istringstream at(line);
        num3(at, &xyz[3 * (size_t)i]);
    }
    return xyz;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: cellgrid_harness CASES\n"); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { fprintf(stderr, "cellgrid_harness: cannot read %s\n", argv[1]); return 2; }
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
            for (int k = 0; k < 3; ++k) g.crs_start[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) g.xyz_interval[k] = (int32_t)integer(in);
            num3(in, g.origin);
            num3(in, g.grid_len);
            for (int k = 0; k < 9; ++k) g.ortho[k] = num(in);
            for (int k = 0; k < 9; ++k) g.deortho[k] = num(in);
        } else if (kind == "grid") {
            double lo[3], hi[3];
            num3(in, lo);
            num3(in, hi);
            const double cutoff = num(in);
            const long long n_points = integer(in);
            CellGrid grid;
            if (make_cell_grid(lo, hi, cutoff, n_points, lo, hi, &grid)) print_grid(grid);
            else printf("refused %d\n", bad_extent(lo, hi));
        } else if (kind == "query") {
            const long long n = integer(in);
            const double cutoff = num(in);
            const long long n_points = integer(in);
            const std::vector<double> xyz = points(file, n);
            CellGrid grid;
            double lo[3], hi[3];
            if (query_grid(xyz.data(), n, cutoff, n_points, &grid, lo, hi)) print_grid(grid);
            else printf("refused %d\n", bad_extent(lo, hi));
        } else if (kind == "crop") {
            double blo[3], bhi[3];
            num3(in, blo);
            num3(in, bhi);
            const double reach = num(in);
            const long long n = integer(in);
            const std::vector<double> xyz = points(file, n);
            CellGrid grid;
            if (!crop_cell_grid(blo, bhi, reach, xyz.data(), n, &grid)) { printf("refused\n"); continue; }
            print_grid(grid);
            printf("held");
            for (long long i = 0; i < n; ++i) printf(" %d", grid_cropped(grid, &xyz[3 * (size_t)i]) ? -1 : grid_cell(grid, &xyz[3 * (size_t)i]));
            printf("\n");
        } else if (kind == "corners") {
            int32_t c0[3], c1[3];
            for (int k = 0; k < 3; ++k) c0[k] = (int32_t)integer(in);
            for (int k = 0; k < 3; ++k) c1[k] = (int32_t)integer(in);
            double lo[3], hi[3];
            crs_box_xyz(g, c0, c1, lo, hi);
            printf("corners");
            print_bits(lo, 3);
            print_bits(hi, 3);
            printf("\n");
        } else if (kind == "reach") {
            printf("reach %d\n", reach_below_2p29_steps(g, num(in)) ? 1 : 0);
        } else {
            fprintf(stderr, "cellgrid_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
