// pdbeda_cloud.h -- the host decisions of pdbeda_aggregate_cloud (densityAnalysis.py:604-731): which atoms are pooled and what every table says,
// on plain arrays.  No HIP call, no device pointer, no context: the file compiles with the host compiler alone and runs under its sanitizers
// (tests/cloud_harness.cpp, tests/test_cloud_decisions_host.py); the device orchestration around the two calls is in pdbeda_hip.hip.
//   cloud_pool()    between the sphere job's table and the union job: cut-off, best cloud, pool, residue groups, voxel offsets, bonded pairs
//   cloud_finish()  behind the union job's one wait: owner states, electrons per union component, emission order, filter, totals
// Both trust what the entry point has checked: alias and key of every atom and every owner key in range, residues in order, a clouds' table
// sorted by group with groups in [0, n).
#pragma once
#include "../../include/pdbeda.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pdbeda {

// numpy's add.reduce over a contiguous float64 array (see k_np_chunk_sums): blocks of 8192 accumulated in order, each a
// pairwise sum.  mode 1: (x - shift)^2.  The centroid-distance cut-off (densityAnalysis.py:607) decides which atoms are
// pooled, so np.nanmedian + 2.5 * np.nanstd is reproduced operation by operation, not approximated (build with -ffp-contract=off).
static double np_elem_h(const double *a, int64_t i, int mode, double shift) {
    double v = a[i];
    if (mode == 1) { v = v - shift; v = v * v; }
    return v;
}
static double np_pairwise_h(const double *a, int64_t off, int64_t n, int mode, double shift) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += np_elem_h(a, off + i, mode, shift);
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = np_elem_h(a, off + j, mode, shift);
        int64_t i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += np_elem_h(a, off + i + j, mode, shift);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += np_elem_h(a, off + i, mode, shift);
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_h(a, off, n2, mode, shift) + np_pairwise_h(a, off + n2, n - n2, mode, shift);
}
static double np_sum_h(const double *a, int64_t n, int mode, double shift) {
    double out = 0.0;
    for (int64_t off = 0; off < n; off += 8192) out += np_pairwise_h(a, off, std::min<int64_t>(8192, n - off), mode, shift);
    return out;
}
static double np_median_h(std::vector<double> v) {   // np.median of a NaN-free 1-D array (the middle order statistics: a selection, not a sort)
    const size_t n = v.size();
    if (n == 0) return NAN;
    std::nth_element(v.begin(), v.begin() + n / 2, v.end());
    const double hi = v[n / 2];
    if (n & 1) return hi;
    const double lo = *std::max_element(v.begin(), v.begin() + n / 2);   // (the largest of what was put below the middle)
    return (lo + hi) / 2.0;
}
static double np_std_h(const std::vector<double> &v) {   // np.std (population) of a NaN-free 1-D array
    const int64_t n = (int64_t)v.size();
    if (n == 0) return NAN;
    const double mean = np_sum_h(v.data(), n, 0, 0.0) / (double)n;
    return std::sqrt(np_sum_h(v.data(), n, 1, mean) / (double)n);
}

static inline double norm3(const double *a, const double *b) {   // np.linalg.norm(a - b): sqrt((dx^2 + dy^2) + dz^2)
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

// The result tables of pdbeda_aggregate_cloud (the opaque pdbeda_cloud handle is these and its context)
struct CloudRow { int32_t residue; double total; int64_t n; double electrons; double cen[3]; };
struct CloudTables {
    std::vector<int32_t> atom_idx;
    std::vector<double> atom_total, atom_centroid, atom_dist;
    std::vector<int64_t> atom_nvox;
    std::vector<CloudRow> res_rows, dom_rows;
    std::vector<uint8_t> owner_state;      // n_owners, zeroed by the caller
    double totals[4] = {0.0, 0.0, 0.0, 0.0};
};

// What cloud_pool() decides for the device and for cloud_finish()
struct CloudPool {
    std::vector<int64_t> first;                             // n + 1: clouds of atom a are [first[a], first[a + 1])  (sorted by group)
    double cutoff = NAN;
    std::vector<int32_t> pool_cloud, pool_atom;             // a pool entry per cloud of every pooled atom, in atom order
    std::vector<int32_t> pool_group, group_res;             // compact residue groups in increasing order, and their residue ordinals
    std::vector<int64_t> pool_voff, set_off;                // n_pool + 1: voxel offsets of the pool entries;  n + 1: voxel slice (all clouds) of every atom
    std::vector<int32_t> pair_a, pair_b, pair_owner;        // bonded pairs between pooled names: the two aliases, and the owner that asks
    int64_t n_pool() const { return (int64_t)pool_cloud.size(); }
    int64_t V() const { return pool_voff.empty() ? 0 : pool_voff.back(); }
};

enum CloudDecision { CLOUD_OK = 0, CLOUD_BONDED_KEY_RANGE = 1, CLOUD_COMPONENT_RANGE = 2 };

static inline double cloud_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Centroid-distance cut-off, best cloud, pool (604-642); then the residue groups, the voxel offsets and the bonded pairs of what was pooled.
// c_*: the sphere job's table (n, total, centroid, group per cloud; a group per atom).  Writes pool, the pooled atoms' rows, totals[3] and the owner
// states 1 into tab.  Nothing pooled: the pool lists stay empty.  CLOUD_BONDED_KEY_RANGE: a pooled owner's bonded list holds a key outside
// [0, n_keys) -- only those lists are read.  marks (experiments, may be null): the times behind the cut-off and behind the pool loop.
static int cloud_pool(const pdbeda_cloud_atoms &at, const std::vector<int64_t> &c_n, const std::vector<double> &c_tot, const std::vector<double> &c_cen,
                      const std::vector<int32_t> &c_grp, CloudPool &pool, CloudTables &tab, double *marks = nullptr) {
    const int64_t n = at.n, nb = (int64_t)c_n.size();
    std::vector<int64_t> &first = pool.first;
    first.assign((size_t)n + 1, 0);
    for (int64_t c = 0; c < nb; ++c) first[(size_t)c_grp[(size_t)c] + 1]++;
    for (int64_t a = 0; a < n; ++a) first[(size_t)a + 1] += first[(size_t)a];
    std::vector<double> c_dist((size_t)nb), min_dist((size_t)n, NAN);
    std::vector<double> centroidDistances;
    centroidDistances.reserve((size_t)n);
    for (int64_t a = 0; a < n; ++a) {
        double mn = NAN;
        for (int64_t c = first[(size_t)a]; c < first[(size_t)a + 1]; ++c) {
            c_dist[(size_t)c] = norm3(at.xyz + 3 * a, c_cen.data() + 3 * c);
            if (c == first[(size_t)a] || c_dist[(size_t)c] < mn) mn = c_dist[(size_t)c];
        }
        min_dist[(size_t)a] = mn;
        if (first[(size_t)a + 1] > first[(size_t)a]) centroidDistances.push_back(mn);
    }
    const double cutoff = np_median_h(centroidDistances) + 2.5 * np_std_h(centroidDistances);
    pool.cutoff = tab.totals[3] = cutoff;
    if (marks) marks[0] = cloud_now_s();
    std::vector<int32_t> &pool_cloud = pool.pool_cloud, &pool_atom = pool.pool_atom;
    pool_cloud.reserve((size_t)nb); pool_atom.reserve((size_t)nb);
    tab.atom_idx.reserve((size_t)n); tab.atom_total.reserve((size_t)n); tab.atom_nvox.reserve((size_t)n);
    tab.atom_centroid.reserve(3 * (size_t)n); tab.atom_dist.reserve((size_t)n);
    std::vector<int32_t> pooled_of_key((size_t)at.n_keys, -1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = at.alias[i], lo = first[(size_t)s], hi = first[(size_t)s + 1];
        if (hi == lo) continue;
        int64_t best = lo;
        if (hi - lo > 1) {
            if (min_dist[(size_t)s] > cutoff) continue;
            for (int64_t c = lo + 1; c < hi; ++c)
                if (c_dist[(size_t)c] < c_dist[(size_t)best]) best = c;      // the first minimum (distances.index(min))
        }
        for (int64_t c = lo; c < hi; ++c) { pool_cloud.push_back((int32_t)c); pool_atom.push_back((int32_t)i); }
        pooled_of_key[(size_t)at.key[i]] = (int32_t)i;                      // the last atom of a name wins (640)
        tab.atom_idx.push_back((int32_t)i);
        tab.atom_total.push_back(c_tot[(size_t)best]);
        tab.atom_nvox.push_back(c_n[(size_t)best]);
        for (int k = 0; k < 3; ++k) tab.atom_centroid.push_back(c_cen[3 * (size_t)best + k]);
        tab.atom_dist.push_back(norm3(at.xyz + 3 * i, c_cen.data() + 3 * best));
    }
    if (marks) marks[1] = cloud_now_s();
    const int64_t n_pool = pool.n_pool();
    if (n_pool == 0) return CLOUD_OK;

    std::vector<int32_t> &group_res = pool.group_res;
    pool.pool_group.resize((size_t)n_pool);
    for (int64_t p = 0; p < n_pool; ++p) {
        const int32_t r = at.residue[pool_atom[(size_t)p]];
        if (group_res.empty() || group_res.back() != r) group_res.push_back(r);
        pool.pool_group[(size_t)p] = (int32_t)group_res.size() - 1;
    }
    pool.pool_voff.assign((size_t)n_pool + 1, 0);
    pool.set_off.assign((size_t)n + 1, 0);
    for (int64_t p = 0; p < n_pool; ++p) pool.pool_voff[(size_t)p + 1] = pool.pool_voff[(size_t)p] + c_n[(size_t)pool_cloud[(size_t)p]];
    {   // voxel slice (all clouds) of every atom inside the sphere job's list, for the overlap tests
        std::vector<int64_t> coff((size_t)nb + 1, 0);
        for (int64_t c = 0; c < nb; ++c) coff[(size_t)c + 1] = coff[(size_t)c] + c_n[(size_t)c];
        for (int64_t a = 0; a <= n; ++a) pool.set_off[(size_t)a] = coff[(size_t)first[(size_t)a]];
    }
    // bonded pairs between pooled names (656): owner o tests its name's atom against every bonded partner that is pooled
    for (int64_t o = 0; o < at.n_owners; ++o) {
        const int32_t k = at.owner_key[o], ia = pooled_of_key[(size_t)k];
        if (ia < 0) continue;
        tab.owner_state[(size_t)o] = 1;
        for (int64_t q = at.bonded_off[k]; q < at.bonded_off[k + 1]; ++q) {
            const int32_t k2 = at.bonded[q];
            if (k2 < 0 || k2 >= at.n_keys) return CLOUD_BONDED_KEY_RANGE;
            const int32_t ib = pooled_of_key[(size_t)k2];
            if (ib < 0) continue;
            pool.pair_a.push_back(at.alias[ia]); pool.pair_b.push_back(at.alias[ib]); pool.pair_owner.push_back((int32_t)o);
        }
    }
    return CLOUD_OK;
}

// Overlap completeness, electrons per union component, emission order, totals (652-731).  u_*: the union job's table (a group per residue
// group of the pool, then the domain group), in any order, every row with a pool entry in it; comp[kind * n_pool + p]: the row of the component that holds pool entry p in its
// residue group (kind 0) and in the domain group (kind 1); touch[q]: pair q's voxel sets touch.  Writes the owner states 2, res_rows,
// dom_rows and totals[0..2] into tab.  CLOUD_COMPONENT_RANGE: a comp outside [0, rows of the table).
static int cloud_finish(const pdbeda_cloud_atoms &at, const CloudPool &pool, const std::vector<int64_t> &u_n, const std::vector<double> &u_tot,
                        const std::vector<double> &u_cen, const std::vector<int32_t> &u_grp, const std::vector<int32_t> &comp,
                        const std::vector<unsigned int> &touch, double min_cloud_electrons, CloudTables &tab) {
    const int64_t n = at.n, n_pool = pool.n_pool(), n_pairs = (int64_t)pool.pair_a.size(), nu = (int64_t)u_n.size();
    const int32_t n_rg = (int32_t)pool.group_res.size();
    const std::vector<int32_t> &pool_atom = pool.pool_atom;
    for (int64_t q = 0; q < n_pairs; ++q)
        if (!touch[(size_t)q]) tab.owner_state[(size_t)pool.pair_owner[(size_t)q]] = 2;
    std::vector<double> electrons((size_t)nu, 0.0);
    std::vector<int64_t> first_pool((size_t)nu, n_pool);
    // Whose electrons a pooled cloud carries (cloud.atoms, 639 / 690 / 718).  The atoms of one coordinate share the cloud OBJECTS
    // of the last of them (605, 622), and the atom loop of a residue overwrites their .atoms (639): when two pooled atoms of ONE
    // residue share a coordinate, both pool entries are the same objects and name only the LATER atom -- the earlier one's
    // electrons are in no residue or domain cloud (golden analysis_alias; round 3 counted both).  Atoms of different residues
    // each get their own residue's snapshot (clone(), 675), so both count there and in the domain.
    std::vector<int32_t> named_by((size_t)n);
    for (int64_t i = 0; i < n; ++i) named_by[(size_t)i] = (int32_t)i;
    {
        std::vector<int32_t> last_of_alias((size_t)n, -1);             // per residue: the last pooled atom that uses the clouds of alias a
        size_t r0 = 0;
        const std::vector<int32_t> &pooled = tab.atom_idx;             // (in atom order, hence residue by residue)
        while (r0 < pooled.size()) {
            size_t r1 = r0;
            while (r1 < pooled.size() && at.residue[pooled[r1]] == at.residue[pooled[r0]]) ++r1;
            for (size_t q = r0; q < r1; ++q) last_of_alias[(size_t)at.alias[pooled[q]]] = pooled[q];
            for (size_t q = r0; q < r1; ++q) named_by[(size_t)pooled[q]] = last_of_alias[(size_t)at.alias[pooled[q]]];
            for (size_t q = r0; q < r1; ++q) last_of_alias[(size_t)at.alias[pooled[q]]] = -1;
            r0 = r1;
        }
    }
    std::vector<std::pair<int32_t, int32_t>> members;                  // (union component, atom named by a pooled cloud in it): distinct pairs add electrons once
    members.reserve(2 * (size_t)n_pool);
    for (int kind = 0; kind < 2; ++kind) {
        for (int64_t p = 0; p < n_pool; ++p) {
            const int32_t k = comp[(size_t)(kind * n_pool + p)];
            if (k < 0 || k >= nu) return CLOUD_COMPONENT_RANGE;
            members.emplace_back(k, named_by[(size_t)pool_atom[(size_t)p]]);
            if (p < first_pool[(size_t)k]) first_pool[(size_t)k] = p;
        }
    }
    {   // (summed in atom order per component, as before: pool order is atom order)
        std::stable_sort(members.begin(), members.end());
        for (size_t q = 0; q < members.size(); ++q)
            if (q == 0 || members[q] != members[q - 1]) electrons[(size_t)members[q].first] += at.weight[members[q].second];
    }
    std::vector<int64_t> order((size_t)nu);
    for (int64_t k = 0; k < nu; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const bool da = u_grp[(size_t)a] == n_rg, db = u_grp[(size_t)b] == n_rg;
        if (da != db) return db;                                   // residue clouds first, then the domain clouds
        return first_pool[(size_t)a] < first_pool[(size_t)b];
    });
    double num_voxels = 0.0, total_electrons = 0.0, total_density = 0.0;
    for (int64_t idx = 0; idx < nu; ++idx) {
        const int64_t k = order[(size_t)idx];
        const bool dom = u_grp[(size_t)k] == n_rg;
        CloudRow row;
        row.total = u_tot[(size_t)k]; row.n = u_n[(size_t)k]; row.electrons = electrons[(size_t)k];
        for (int q = 0; q < 3; ++q) row.cen[q] = u_cen[3 * (size_t)k + q];
        if (dom) {
            total_electrons += row.electrons;
            num_voxels += (double)row.n;
            total_density += row.total;
            row.residue = at.residue[pool_atom[(size_t)first_pool[(size_t)k]]];
            if (row.electrons >= min_cloud_electrons) tab.dom_rows.push_back(row);
        } else {
            row.residue = pool.group_res[(size_t)u_grp[(size_t)k]];
            if (row.electrons >= min_cloud_electrons) tab.res_rows.push_back(row);
        }
    }
    tab.totals[0] = num_voxels; tab.totals[1] = total_electrons; tab.totals[2] = total_density;
    return CLOUD_OK;
}

}  // namespace pdbeda
