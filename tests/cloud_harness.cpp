// tests/cloud_harness.cpp -- the host decisions of pdbeda_aggregate_cloud (pdb_eda_amd/csrc/pdbeda_cloud.h) as a stand-alone program.
//
// Test infrastructure (CPU): tests/test_cloud_decisions_host.py writes cases into a text file, builds this file with the host compiler under
// AddressSanitizer + UBSan (and -ffp-contract=off, as the library), runs it and reads the result file.  Every array has exactly the size its
// record names and an empty one is a null pointer, so a read past one is the sanitizer's to report.  The case file is a stream of
// whitespace-separated tokens, doubles as C99 hex floats (or nan / inf); a record is a word and what follows it:
//   sum MODE SHIFT N x...      np_sum_h(x, N, MODE, SHIFT)                                          -> "sum X"
//   std N x... | median N x... np_std_h / np_median_h                                               -> "std X" | "median X"
//   norm3 a0 a1 a2 b0 b1 b2                                                                          -> "norm3 X"
//   atoms N NKEYS NOWNERS NBONDED  xyz[3N] weight[N] residue[N] alias[N] key[N] bonded_off[NKEYS + 1, none if NKEYS = 0] bonded[NBONDED] owner_key[NOWNERS]
//                              the pdbeda_cloud_atoms of the records that follow (radius: null, no decision reads it)
//   clouds NB  n[NB] total[NB] centroid[3NB] group[NB]      the sphere job's table
//   pool                       cloud_pool() on fresh tables (owners in state 0, totals 0 0 0 nan)   -> "pool RC" and, one line each as "name COUNT values...",
//                              cutoff first pool_cloud pool_atom pool_group group_res pool_voff set_off pair_a pair_b pair_owner owner_state
//                              atom_idx atom_total atom_nvox atom_centroid atom_dist
//   finish NU u_n[NU] u_total[NU] u_centroid[3NU] u_group[NU] comp[2 n_pool] touch[n_pairs] MIN_ELECTRONS
//                              cloud_finish() on the pool and the tables of the last pool record     -> "finish RC", owner_state, totals (the four),
//                              and per table res_* / dom_*: residue total n electrons centroid
#include "pdbeda_cloud.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

using namespace pdbeda;

namespace {

std::ifstream in;
FILE *out = nullptr;

std::string word() {
    std::string w;
    if (!(in >> w)) { fprintf(stderr, "cloud_harness: the case file ends inside a record\n"); exit(2); }
    return w;
}
double real() {
    const std::string w = word();
    char *end = nullptr;
    const double v = strtod(w.c_str(), &end);
    if (end == w.c_str() || *end) { fprintf(stderr, "cloud_harness: '%s' is no number\n", w.c_str()); exit(2); }
    return v;
}
long long integer() {
    const std::string w = word();
    char *end = nullptr;
    const long long v = strtoll(w.c_str(), &end, 10);
    if (end == w.c_str() || *end) { fprintf(stderr, "cloud_harness: '%s' is no integer\n", w.c_str()); exit(2); }
    return v;
}
template <typename T> std::vector<T> integers(size_t n) {
    std::vector<T> v(n);
    for (T &x : v) x = (T)integer();
    v.shrink_to_fit();
    return v;
}
std::vector<double> reals(size_t n) {
    std::vector<double> v(n);
    for (double &x : v) x = real();
    v.shrink_to_fit();
    return v;
}
template <typename T> const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

template <typename T> void put_ints(const char *name, const std::vector<T> &v) {
    fprintf(out, "%s %zu", name, v.size());
    for (const T &x : v) fprintf(out, " %lld", (long long)x);
    fprintf(out, "\n");
}
void put_reals(const char *name, const double *v, size_t n) {
    fprintf(out, "%s %zu", name, n);
    for (size_t i = 0; i < n; ++i) fprintf(out, " %a", v[i]);
    fprintf(out, "\n");
}
void put_reals(const char *name, const std::vector<double> &v) { put_reals(name, v.data(), v.size()); }
void put_rows(const std::string &tag, const std::vector<CloudRow> &rows) {
    std::vector<int32_t> residue;
    std::vector<int64_t> n;
    std::vector<double> total, electrons, centroid;
    for (const CloudRow &r : rows) {
        residue.push_back(r.residue); n.push_back(r.n); total.push_back(r.total); electrons.push_back(r.electrons);
        centroid.insert(centroid.end(), r.cen, r.cen + 3);
    }
    put_ints((tag + "_residue").c_str(), residue); put_reals((tag + "_total").c_str(), total); put_ints((tag + "_n").c_str(), n);
    put_reals((tag + "_electrons").c_str(), electrons); put_reals((tag + "_centroid").c_str(), centroid);
}

struct Atoms {
    std::vector<double> xyz, weight;
    std::vector<int32_t> residue, alias, key, bonded, owner_key;
    std::vector<int64_t> bonded_off;
    pdbeda_cloud_atoms at;
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: cloud_harness CASES RESULTS\n"); return 2; }
    in.open(argv[1]);
    if (!in) { fprintf(stderr, "cloud_harness: cannot read %s\n", argv[1]); return 2; }
    out = fopen(argv[2], "w");
    if (!out) { fprintf(stderr, "cloud_harness: cannot write %s\n", argv[2]); return 2; }
    Atoms a;
    a.at = pdbeda_cloud_atoms();
    std::vector<int64_t> c_n;
    std::vector<double> c_tot, c_cen;
    std::vector<int32_t> c_grp;
    CloudPool pool;
    CloudTables tab;
    std::string kind;
    while (in >> kind) {
        if (kind == "sum") {
            const int mode = (int)integer();
            const double shift = real();
            const std::vector<double> x = reals((size_t)integer());
            put_reals("sum", std::vector<double>{np_sum_h(ptr(x), (int64_t)x.size(), mode, shift)});
        } else if (kind == "std" || kind == "median") {
            const std::vector<double> x = reals((size_t)integer());
            put_reals(kind.c_str(), std::vector<double>{kind == "std" ? np_std_h(x) : np_median_h(x)});
        } else if (kind == "norm3") {
            const std::vector<double> x = reals(6);
            put_reals("norm3", std::vector<double>{norm3(x.data(), x.data() + 3)});
        } else if (kind == "atoms") {
            const size_t n = (size_t)integer(), n_keys = (size_t)integer(), n_owners = (size_t)integer(), n_bonded = (size_t)integer();
            a.xyz = reals(3 * n); a.weight = reals(n);
            a.residue = integers<int32_t>(n); a.alias = integers<int32_t>(n); a.key = integers<int32_t>(n);
            a.bonded_off = integers<int64_t>(n_keys ? n_keys + 1 : 0); a.bonded = integers<int32_t>(n_bonded); a.owner_key = integers<int32_t>(n_owners);
            a.at.n = (int64_t)n; a.at.n_keys = (int64_t)n_keys; a.at.n_owners = (int64_t)n_owners;
            a.at.xyz = ptr(a.xyz); a.at.radius = nullptr; a.at.weight = ptr(a.weight); a.at.residue = ptr(a.residue); a.at.alias = ptr(a.alias);
            a.at.key = ptr(a.key); a.at.bonded_off = ptr(a.bonded_off); a.at.bonded = ptr(a.bonded); a.at.owner_key = ptr(a.owner_key);
        } else if (kind == "clouds") {
            const size_t nb = (size_t)integer();
            c_n = integers<int64_t>(nb); c_tot = reals(nb); c_cen = reals(3 * nb); c_grp = integers<int32_t>(nb);
        } else if (kind == "pool") {
            pool = CloudPool();
            tab = CloudTables();
            tab.owner_state.assign((size_t)a.at.n_owners, 0);
            tab.totals[3] = NAN;
            fprintf(out, "pool %d\n", cloud_pool(a.at, c_n, c_tot, c_cen, c_grp, pool, tab));
            put_reals("cutoff", &pool.cutoff, 1);
            put_ints("first", pool.first); put_ints("pool_cloud", pool.pool_cloud); put_ints("pool_atom", pool.pool_atom);
            put_ints("pool_group", pool.pool_group); put_ints("group_res", pool.group_res); put_ints("pool_voff", pool.pool_voff);
            put_ints("set_off", pool.set_off); put_ints("pair_a", pool.pair_a); put_ints("pair_b", pool.pair_b); put_ints("pair_owner", pool.pair_owner);
            put_ints("owner_state", tab.owner_state);
            put_ints("atom_idx", tab.atom_idx); put_reals("atom_total", tab.atom_total); put_ints("atom_nvox", tab.atom_nvox);
            put_reals("atom_centroid", tab.atom_centroid); put_reals("atom_dist", tab.atom_dist);
        } else if (kind == "finish") {
            const size_t nu = (size_t)integer();
            const std::vector<int64_t> u_n = integers<int64_t>(nu);
            const std::vector<double> u_tot = reals(nu), u_cen = reals(3 * nu);
            const std::vector<int32_t> u_grp = integers<int32_t>(nu), comp = integers<int32_t>(2 * (size_t)pool.n_pool());
            const std::vector<unsigned int> touch = integers<unsigned int>(pool.pair_a.size());
            const double min_electrons = real();
            fprintf(out, "finish %d\n", cloud_finish(a.at, pool, u_n, u_tot, u_cen, u_grp, comp, touch, min_electrons, tab));
            put_ints("owner_state", tab.owner_state);
            put_reals("totals", tab.totals, 4);
            put_rows("res", tab.res_rows); put_rows("dom", tab.dom_rows);
        } else {
            fprintf(stderr, "cloud_harness: unknown record '%s'\n", kind.c_str());
            return 2;
        }
    }
    if (fclose(out) != 0) { fprintf(stderr, "cloud_harness: cannot finish %s\n", argv[2]); return 2; }
    return 0;
}
