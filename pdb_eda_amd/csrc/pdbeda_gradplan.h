// pdbeda_gradplan.h -- the host's plan of pdbeda_atom_moments: the argument checks, the box of crs indices that covers an atom's sphere on ANY
// cell, clipped to the domain, and the quantum of the integer sums.  Plain integers and doubles -- no HIP call, no pointer into device memory:
// the file compiles with the host compiler alone and runs under its sanitizers (tests/gradient_harness.cpp); the caller is pdbeda_atom_moments
// in pdbeda_hip.hip, and pdbeda_gradient.h includes this file for the box record.  The contract: include/pdbeda.h.
//
// The box.  rows[k] is row k of the xyz -> crs matrix (grid steps of crs axis k per Angstrom along x, y, z), off[k] its offset: a point p lies at
// the grid position f_k = rows[k] . p + off[k].  atom_box of pdbeda_spherebox.h (the reference's rule: xyz2crs of origin + radius) is NOT a
// covering rule on a skewed cell and is not used.  THE PROOF, in two lines: for a voxel v inside the sphere, |v_k - f_k| = |rows[k] . (p_v - x)| <=
// |rows[k]|_2 |p_v - x| <= |rows[k]|_2 r = h_k (Cauchy-Schwarz); every fp64 step between the kernel's test and this f_k and h_k (crs2xyz, d2, the
// root, the dot products, the inverse matrix) is off by less than 2^-45 of the magnitudes that enter it, and the box is widened by 2^-30 of
// their sum (GP_PAD): 2^15 times as much, at the price of one more plane of voxels for about one atom in 2^28.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "pdbeda_jobplan.h"

namespace pdbeda {

constexpr int GP_MAX_TERMS = 6;              // == PDBEDA_MODEL_MAX_TERMS
constexpr double GP_PAD = 0x1p-30;           // the widening of a half-width, relative to everything that was rounded on the way to it
constexpr int GP_WAVES = 4;                  // atoms of a workgroup of 256: a wave each
constexpr int GP_COLS = 16, GP_ROWS = 4;     // the voxels of one trip of a wave: 16 along c times 4 along r

// What stands in the call's way, in the order the checks run (the first that applies).
enum : int {
    GRAD_OK = 0,
    GRAD_TERMS = 1,       // n_terms outside 1 .. GP_MAX_TERMS
    GRAD_FLAG = 2,        // an unknown flag
    GRAD_COUNT = 3,       // 2^31 atoms or more (or a negative number of them)
    GRAD_XYZ = 4,         // a non-finite coordinate
    GRAD_EXPO = 5,        // a non-finite or negative exponent
    GRAD_RADIUS = 6,      // a radius that is not finite or <= 0
    GRAD_REACH = 7,       // a radius of 2^29 grid steps or more along a crs axis
    GRAD_BOX = 8          // a clipped box of 2^31 voxels or more
};

// The checks that need neither the grid nor the device.  *at gets the atom that is refused (-1: none); *r_top the largest radius.
static inline int grad_check(const double *xyz, int64_t n_atoms, int32_t n_terms, const double *expo, const float *radii, uint32_t flags, uint32_t known_flags,
                             int64_t *at, float *r_top) {
    *at = -1;
    *r_top = 0.0f;
    if (n_terms < 1 || n_terms > GP_MAX_TERMS) return GRAD_TERMS;
    if (flags & ~known_flags) return GRAD_FLAG;
    if (n_atoms < 0 || n_atoms >= (1ll << 31)) return GRAD_COUNT;
    for (int64_t i = 0; i < 3 * n_atoms; ++i)
        if (!std::isfinite(xyz[i])) { *at = i / 3; return GRAD_XYZ; }
    for (int64_t i = 0; i < n_atoms * n_terms; ++i)
        if (!std::isfinite(expo[i]) || expo[i] < 0.0) { *at = i / n_terms; return GRAD_EXPO; }
    for (int64_t i = 0; i < n_atoms; ++i) {
        if (!std::isfinite(radii[i]) || !(radii[i] > 0.0f)) { *at = i; return GRAD_RADIUS; }
        *r_top = std::max(*r_top, radii[i]);
    }
    return GRAD_OK;
}

// The grid as the plan sees it: the xyz -> crs map and the domain (the stored box ncrs, or the non-repeating box).
struct GradGrid {
    double rows[9];      // rows[3 k + i]: grid steps of crs axis k per unit of xyz axis i
    double off[3];
    double norm[3];      // |rows[k]|_2 = sqrt((a a + b b) + c c)
    int32_t dom[3];      // voxels of the domain along c, r, s: indices 0 .. dom - 1
};
static inline void grad_grid_norms(GradGrid *g) {
    for (int k = 0; k < 3; ++k) {
        const double a = g->rows[3 * k], b = g->rows[3 * k + 1], c = g->rows[3 * k + 2];
        g->norm[k] = std::sqrt((a * a + b * b) + c * c);
    }
}
// The largest radius spans fewer than 2^29 steps of every crs axis (h_k of the proof): what the casts below rely on.
static inline bool grad_reach_ok(const GradGrid &g, double r_max) {
    for (int k = 0; k < 3; ++k)
        if (!(r_max * g.norm[k] < (double)(1ll << 29))) return false;
    return true;
}

// An atom's clipped box: voxels lo .. lo + n - 1 along c, r, s; n = {0, 0, 0} and lo = {0, 0, 0} when no voxel of the domain can lie in the sphere.
struct GradBox {
    int32_t lo[3];
    int32_t n[3];
};
// The covering range of crs axis k BEFORE any clipping, as doubles: voxels ceil(f - w) .. floor(f + w) (f, h and the widening w of the proof above).
// false: the grid position or the half-width is not finite.  (pdbeda_poseplan.h builds its unclipped, wrap-aware box on this.)
static inline bool grad_span(const GradGrid &g, const double xyz[3], double radius, int k, double *first, double *last) {
    const double t0 = g.rows[3 * k] * xyz[0], t1 = g.rows[3 * k + 1] * xyz[1], t2 = g.rows[3 * k + 2] * xyz[2];
    const double f = ((t0 + t1) + t2) + g.off[k];
    const double h = radius * g.norm[k];
    const double mag = (((std::fabs(t0) + std::fabs(t1)) + std::fabs(t2)) + std::fabs(g.off[k])) + (h + 1.0);
    const double w = h + GP_PAD * mag;
    if (!std::isfinite(f) || !std::isfinite(w)) return false;
    *first = std::ceil(f - w);
    *last = std::floor(f + w);
    return true;
}
// *clipped: the covering box reaches beyond the domain on some axis (an atom wholly outside included).  Returns the box's voxels.
static inline int64_t grad_box(const GradGrid &g, const double xyz[3], double radius, GradBox *box, bool *clipped) {
    double lo[3], hi[3];
    bool empty = false;
    *clipped = false;
    for (int k = 0; k < 3; ++k) {
        double first = 0.0, last = 0.0;
        if (!grad_span(g, xyz, radius, k, &first, &last)) { empty = true; *clipped = true; lo[k] = 0.0; hi[k] = -1.0; continue; }
        const double top = (double)g.dom[k] - 1.0;
        if (first < 0.0 || last > top) *clipped = true;
        lo[k] = std::max(first, 0.0);
        hi[k] = std::min(last, top);
        if (!(lo[k] <= hi[k])) empty = true;
    }
    if (empty) {
        for (int k = 0; k < 3; ++k) box->lo[k] = box->n[k] = 0;
        return 0;
    }
    int64_t vox = 1;
    for (int k = 0; k < 3; ++k) {      // (0 <= lo <= hi < dom < 2^31: the casts are defined)
        box->lo[k] = (int32_t)lo[k];
        box->n[k] = (int32_t)(hi[k] - lo[k]) + 1;
        vox *= box->n[k];
    }
    return vox;
}

static inline bool grad_box_too_large(int64_t voxels) { return voxels >= (1ll << 31); }      // GRAD_BOX: the kernel counts an atom's pairs in 32 bits

// The shift of the integer sums: quantum_shift (pdbeda_jobplan.h) of B = max|w| * max(1, r_max^2) * max(V_max, 2^22).  |w e| <= |w|, |dx| <= r and
// d2 <= r^2 (1 + 2^-50) inside the sphere, so no sum of V_max terms exceeds B (1 + 2^-50), and B * 2^S < 2^61 leaves two bits.
static inline int grad_shift(double max_abs_w, double r_max, int64_t v_max) {
    const double reach = std::max(1.0, r_max * r_max);
    return quantum_shift((max_abs_w * reach) * (double)std::max<int64_t>(v_max, 1ll << 22));
}

}  // namespace pdbeda
