// pdbeda_spherebox.h -- the sphere box and volume rule (getSphereCrsFromXyz, cutils.pyx:220-248), and the host's planner of sphere batches built on it.
// Host and device code: hipcc compiles it into the kernels (pdbeda_kernels.h), a plain C++17 compiler into the host library's planning and into
// tests/spherebox_harness.cpp, which runs the planner on a CPU under sanitizers.
#pragma once
#include "pdbeda_device.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pdbeda {

struct VolDesc {
    int32_t dim[3];     // voxels along c, r, s
    int32_t org[3];     // raw crs of local voxel (0,0,0)
    int32_t row_words;  // ceil(dim[0] / 64)
    int32_t group;      // caller-visible group id (plane for whole-map jobs)
    int64_t word_base;  // first mask word of this volume
    int64_t key_base;   // first key bit of this volume (key = (c*dim[1] + r)*dim[2] + s)
};

struct AtomBox {
    int32_t lo[3];
    int32_t hi[3];  // inclusive; hi < lo => empty
};

// The sphere box and volume rule, stated ONCE for host and device (like xyz2crs: the same IEEE / int32 operations in the same order on both sides, so
// the host may size and lay out a batch without asking the device -- group_setup, pdbeda_aggregate_cloud -- and k_make_vols' check of its totals holds).
// R = xyz2crs(origin + radius): the box's half-widths follow from the radius alone.
__host__ __device__ inline void sphere_half_widths(const Geom &g, double rad, int32_t R[3]) {
    const double o[3] = {g.origin[0] + rad, g.origin[1] + rad, g.origin[2] + rad};
    xyz2crs(g, o, R);
}
// An atom's box is [C - R - 1, C + R] in int32, C = xyz2crs(centre) (Q4); a box empty along any axis becomes lo 0 / hi -1 along all.  false: empty.
__host__ __device__ inline bool atom_box(const int32_t C[3], const int32_t R[3], AtomBox *out) {
    AtomBox bx;
    bool empty = false;
    for (int k = 0; k < 3; ++k) {
        bx.lo[k] = C[k] - R[k] - 1;
        bx.hi[k] = C[k] + R[k];
        empty = empty || (bx.hi[k] < bx.lo[k]);
    }
    if (empty) { for (int k = 0; k < 3; ++k) { bx.lo[k] = 0; bx.hi[k] = -1; } }
    *out = bx;
    return !empty;
}
// A group's inclusive bounds (int32, or the int64 of aggregateCloud's unions; hi < lo along any axis: no voxel) -> its volume descriptor at the running
// word / key bases, and the mask words and keys it adds to them.  An empty group is an all-zero volume.  A width is taken in int64 and stored as int32,
// which IS k_make_vols' int32 `hi - lo + 1` for every input; false: a width of 2^30 voxels or more (the host's builders then leave the batch to the device).
template <typename B>
__host__ __device__ inline bool vol_from_bounds(const B *lo, const B *hi, int32_t group, int64_t word_base, int64_t key_base, VolDesc *out, int64_t *words, int64_t *keys) {
    VolDesc vd;
    bool empty = false, fits = true;
    for (int k = 0; k < 3; ++k) empty = empty || hi[k] < lo[k];
    for (int k = 0; k < 3; ++k) {
        const int64_t d = empty ? 0 : (int64_t)hi[k] - (int64_t)lo[k] + 1;
        fits = fits && d < (1ll << 30);
        vd.org[k] = empty ? 0 : (int32_t)lo[k];
        vd.dim[k] = (int32_t)d;
    }
    vd.row_words = (vd.dim[0] + 63) / 64;
    vd.group = group;
    vd.word_base = word_base;
    vd.key_base = key_base;
    *out = vd;
    *words = (int64_t)vd.row_words * vd.dim[1] * vd.dim[2];
    *keys = (int64_t)vd.dim[0] * vd.dim[1] * vd.dim[2];
    return fits;
}

// ------------------------------------------------------------------------------------
// The host's planner: boxes, volume descriptors and totals of a sphere batch without asking the device -- its twin of k_init_bounds + k_atom_boxes +
// k_make_vols, on the statements above.  Every sphere entry point of the host library sizes its batches here, under one range test and one limit.
// ------------------------------------------------------------------------------------
// The host casts only what it has tested (a cast of a NaN, or of a double outside the integer's range, is undefined on the host; the device's
// conversion saturates): a coordinate is PLANNABLE when its grid positions are finite and every index is below 2^29 in magnitude, a radius when it is
// finite, >= 0 and its half-widths are.  Then neither C - R - 1 nor C + R leaves int32.  What is not plannable is left to the device's own sizing.
constexpr int64_t PLAN_INDEX_LIMIT = 1ll << 29;
// The one limit on what the host lays out: every width of a volume below 2^30 voxels (vol_from_bounds), a volume's rows below 2^31, and the batch
// below 2^31 mask words and 2^40 keys.  Beyond it the batch is left to the device, which sizes and reports.
constexpr int64_t PLAN_WIDTH_LIMIT = 1ll << 30, PLAN_WORDS_LIMIT = 1ll << 31, PLAN_KEYS_LIMIT = 1ll << 40;

// xyz2crs with the range test in front of each cast.  false: not plannable (crs is then not to be read).
inline bool plan_crs(const Geom &g, const double xyz[3], int32_t crs[3]) {
    int64_t wide[3];
    // (2^40: a NaN fails too; the cast, and the index less the map's start, stay far inside int64)
    if (!xyz2crs_if(g, xyz, wide, [](double pos) { return std::fabs(pos) < 1099511627776.0; })) return false;
    for (int k = 0; k < 3; ++k) {
        if (wide[k] <= -PLAN_INDEX_LIMIT || wide[k] >= PLAN_INDEX_LIMIT) return false;
        crs[k] = (int32_t)wide[k];
    }
    return true;
}
// sphere_half_widths for a plannable radius (the same point, origin + radius, through the same xyz2crs).
inline bool plan_half_widths(const Geom &g, float rad, int32_t R[3]) {
    if (!std::isfinite(rad) || !(rad >= 0.0f)) return false;
    const double o[3] = {g.origin[0] + (double)rad, g.origin[1] + (double)rad, g.origin[2] + (double)rad};
    return plan_crs(g, o, R);
}
// The planner's box function: the box of a plannable atom, R from plan_half_widths.  false: not plannable (the box is left empty).
inline bool plan_atom_box(const Geom &g, const double xyz[3], const int32_t R[3], AtomBox *out) {
    int32_t C[3];
    if (!plan_crs(g, xyz, C)) { *out = AtomBox{{0, 0, 0}, {-1, -1, -1}}; return false; }
    (void)atom_box(C, R, out);
    return true;
}

// A plan in the making and, finished, what the host knows of the batch.  push() is the finish of every plan: inclusive bounds of one volume after the
// other -> VolDesc at the running bases, the totals, and the ONE statement of what fits.  Nothing is laid out behind a volume that does not fit.
struct SpherePlan {
    VolDesc *vols = nullptr;       // where the descriptors go (nullptr: totals only)
    int small_rows = 0;            // (ATOM_WORDS: the rows of a box k_atom_engine holds)
    int64_t words = 0, keys = 0;   // the batch's totals: mask words, keys
    int64_t largest = 0;           // voxels of its largest volume
    bool plannable = true;         // every coordinate and radius passed the range test
    bool fits = true;              // plannable, and inside the one limit: only then are boxes, volumes and totals complete
    bool small_boxes = true;       // every volume is one mask word a row and at most small_rows rows
    template <typename B>
    void push(const B *lo, const B *hi, int64_t group) {
        if (!fits) return;
        int64_t d[3] = {0, 0, 0};
        if (!(hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]))
            for (int k = 0; k < 3; ++k) d[k] = (int64_t)hi[k] - (int64_t)lo[k] + 1;
        // (widths first, then rows: no product below, nor in vol_from_bounds, can leave int64)
        fits = d[0] < PLAN_WIDTH_LIMIT && d[1] < PLAN_WIDTH_LIMIT && d[2] < PLAN_WIDTH_LIMIT && d[1] * d[2] < PLAN_WORDS_LIMIT;
        if (!fits) return;
        VolDesc vd;
        int64_t w = 0, k = 0;
        (void)vol_from_bounds(lo, hi, (int32_t)group, words, keys, &vd, &w, &k);
        if (vols) vols[group] = vd;
        small_boxes = small_boxes && vd.row_words <= 1 && (int64_t)vd.dim[1] * vd.dim[2] <= small_rows;
        largest = std::max(largest, k);
        words += w;
        keys += k;
        fits = words < PLAN_WORDS_LIMIT && keys < PLAN_KEYS_LIMIT;
    }
};

// The box around the boxes of each group's atoms (what k_atom_boxes' atomic min / max make on the device).
struct GroupBounds {
    std::vector<int64_t> lo, hi;
    explicit GroupBounds(int64_t n_groups) : lo(3 * (size_t)n_groups, INT64_MAX), hi(3 * (size_t)n_groups, INT64_MIN) {}
    void add(const AtomBox &bx, int64_t group) {
        if (bx.hi[0] < bx.lo[0]) return;      // (atom_box: an empty box is empty along every axis)
        for (int k = 0; k < 3; ++k) {
            lo[3 * (size_t)group + k] = std::min<int64_t>(lo[3 * (size_t)group + k], bx.lo[k]);
            hi[3 * (size_t)group + k] = std::max<int64_t>(hi[3 * (size_t)group + k], bx.hi[k]);
        }
    }
    void finish(SpherePlan &plan) const {      // (a group nothing was added to keeps its sentinels: hi < lo, an all-zero volume)
        for (size_t g = 0; 3 * g < lo.size(); ++g) plan.push(&lo[3 * g], &hi[3 * g], (int64_t)g);
    }
};

// A sphere batch: every atom's box into boxes[n_items], the groups' volumes into vols[n_groups], the totals.  item_group == nullptr: a group per atom
// -- atom a's volume is its box.  xyz == nullptr: from the radii alone -- a box's SIZE follows from its radius, so the box of an atom at index 0 stands
// for every atom of that radius, and no coordinate is converted (plan_radii_totals).
inline SpherePlan plan_spheres(const Geom &g, const double *xyz, const float *radii, const int32_t *item_group, int64_t n_items, int64_t n_groups,
                               AtomBox *boxes, VolDesc *vols, int small_rows) {
    SpherePlan plan{vols, small_rows};
    GroupBounds bounds(item_group ? n_groups : 0);
    const int32_t index0[3] = {0, 0, 0};
    float cached_rad = NAN;      // (a handful of distinct radii, one per atom type: the half-widths are made once per run of equal radii)
    bool ok = false;
    int32_t R[3] = {0, 0, 0};
    AtomBox bx = {{0, 0, 0}, {-1, -1, -1}};
    for (int64_t a = 0; a < n_items; ++a) {
        if (!(radii[a] == cached_rad)) {
            ok = plan_half_widths(g, radii[a], R);
            if (ok && !xyz) (void)atom_box(index0, R, &bx);
            cached_rad = radii[a];
        }
        if (!ok || (xyz && !plan_atom_box(g, xyz + 3 * a, R, &bx))) { plan.plannable = plan.fits = false; return plan; }
        if (boxes) boxes[a] = bx;
        if (item_group) bounds.add(bx, item_group[a]);
        else plan.push(bx.lo, bx.hi, a);
    }
    bounds.finish(plan);
    return plan;
}
// For the one path on which the device makes the boxes and k_make_vols holds its totals against the host's (a batch too large to stage stays cheap).
inline SpherePlan plan_radii_totals(const Geom &g, const float *radii, int64_t n_items, int small_rows) {
    return plan_spheres(g, nullptr, radii, nullptr, n_items, n_items, nullptr, nullptr, small_rows);
}

}  // namespace pdbeda
