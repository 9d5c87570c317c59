// pdbeda_poseplan.h -- the host's plan of pdbeda_pose_scores: the argument checks in their order, the fragment's radius, the box of crs indices a
// centre's poses can read, the staged-or-global decision against the LDS budget, the chunking of the centres and the carve of the call's scratch.
// Plain integers, doubles and pointers that are never followed -- no HIP call: the file compiles with the host compiler alone and runs under its
// sanitizers (tests/pose_harness.cpp); the caller is pdbeda_pose_scores in pdbeda_hip.hip, and pdbeda_pose.h includes this file for the box record.
// The contract: include/pdbeda.h.
//
// The box.  Every atom of every pose of a centre c lies within r = max_a |x_a| of c when the rotation is orthonormal, so its grid position lies in
// grad_span's covering range of the sphere (c, r) -- the rule of pdbeda_gradplan.h, which holds on skewed cells; it is reused, not restated.  The
// interpolation reads floor(f) and floor(f) + 1: one voxel below the range and one above; one more voxel of safety on either side takes in what
// the kernel's own fp64 (the rounded rotation, the rounded sum c + R x, xyz2frac's dot product against the plan's) can move a position by -- far
// less than a voxel.  NOTHING DEPENDS ON THE BOX BUT THE SPEED: rotations are not checked for orthonormality, and a lane whose eight corners are
// not all inside the staged box reads the map directly, with the same arithmetic and the same bytes out.  The box is NOT clipped: it may reach
// beyond the stored voxels and is filled through the wrap rule, voxel by voxel.
#pragma once
#include "pdbeda_gradplan.h"
#include "pdbeda_stage.h"

namespace pdbeda {

constexpr int POSE_MAX_ATOMS = 256;                 // == PDBEDA_POSE_MAX_ATOMS
constexpr int POSE_MAX_ROTATIONS = 1 << 20;         // == PDBEDA_POSE_MAX_ROTATIONS
constexpr int POSE_MAX_TOP = 64;                    // == PDBEDA_POSE_MAX_TOP
constexpr int POSE_LDS_BUDGET = 128 * 1024;         // bytes of LDS a centre's box may take (values + stored bits); a CU has 160 KiB
constexpr int POSE_GROW = 2;                        // voxels the covering range is grown by on either side: the interpolation support and one of safety
constexpr int64_t POSE_TABLE_BYTES = (int64_t)64 << 20;      // what the score table of one chunk of centres may take
constexpr int POSE_TABLE_ROW = 8 + 4 + 1;           // bytes of the table per pose: score, low atoms, kept

// What stands in the call's way, in the order the checks run (the first that applies).
enum : int {
    POSE_OK = 0,
    POSE_ATOMS = 1,          // n_frag outside 1 .. POSE_MAX_ATOMS
    POSE_ROTATIONS = 2,      // n_rot outside 1 .. POSE_MAX_ROTATIONS
    POSE_TOP = 3,            // top_k outside 1 .. POSE_MAX_TOP
    POSE_FLAG = 4,           // an unknown flag
    POSE_COUNT = 5,          // a negative number of centres, or n_centres * n_rot >= 2^31
    POSE_FRAG_VALUE = 6,     // a non-finite fragment coordinate or weight
    POSE_ROT_VALUE = 7,      // a non-finite rotation entry
    POSE_CENTRE_VALUE = 8,   // a non-finite centre
    POSE_REACH = 9,          // the fragment's radius spans 2^29 grid steps or more along a crs axis
    POSE_CENTRE_GRID = 10    // a centre whose grid position is 2^29 steps or more
};

// The checks that need no grid.  *at gets the atom, rotation or centre that is refused (-1: none); *radius the fragment's, max_a sqrt((x x + y y) + z z).
static inline int pose_check(const double *frag_xyz, const double *frag_w, int32_t n_frag, const double *rot, int64_t n_rot, const double *centres, int64_t n_centres,
                             int32_t top_k, uint32_t flags, uint32_t known_flags, int64_t *at, double *radius) {
    *at = -1;
    *radius = 0.0;
    if (n_frag < 1 || n_frag > POSE_MAX_ATOMS) return POSE_ATOMS;
    if (n_rot < 1 || n_rot > POSE_MAX_ROTATIONS) return POSE_ROTATIONS;
    if (top_k < 1 || top_k > POSE_MAX_TOP) return POSE_TOP;
    if (flags & ~known_flags) return POSE_FLAG;
    if (n_centres < 0 || n_centres >= (1ll << 31) || n_centres * n_rot >= (1ll << 31)) return POSE_COUNT;
    for (int32_t a = 0; a < n_frag; ++a) {
        const double x = frag_xyz[3 * a], y = frag_xyz[3 * a + 1], z = frag_xyz[3 * a + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !std::isfinite(frag_w[a])) { *at = a; return POSE_FRAG_VALUE; }
        *radius = std::max(*radius, std::sqrt((x * x + y * y) + z * z));
    }
    for (int64_t i = 0; i < 9 * n_rot; ++i)
        if (!std::isfinite(rot[i])) { *at = i / 9; return POSE_ROT_VALUE; }
    for (int64_t i = 0; i < 3 * n_centres; ++i)
        if (!std::isfinite(centres[i])) { *at = i / 3; return POSE_CENTRE_VALUE; }
    return POSE_OK;
}

// The grid position of a centre stays below 2^29 in magnitude on every axis (the plan's own f: rows . c + off).
static inline bool pose_centre_ok(const GradGrid &g, const double c[3]) {
    for (int k = 0; k < 3; ++k) {
        const double f = ((g.rows[3 * k] * c[0] + g.rows[3 * k + 1] * c[1]) + g.rows[3 * k + 2] * c[2]) + g.off[k];
        if (!(std::fabs(f) < (double)(1ll << 29))) return false;
    }
    return true;
}

// A centre's box: voxels lo .. lo + n - 1 along c, r, s (raw indices: they may lie outside the stored box), and whether the kernel stages it.
struct PoseBox {
    int32_t lo[3];
    int32_t n[3];
    int32_t staged;
    int32_t pad;
};
static inline int64_t pose_lds_bytes(int64_t voxels) { return 4 * voxels + 8 * ((voxels + 63) / 64); }      // float values, then a stored BIT per voxel
// The box of a centre that pose_centre_ok accepts under a radius that grad_reach_ok accepts (|lo| < 2^30 + 3, n < 2^30 + 6: the casts are defined).
// Returns the box's voxels, or -1 for a box with a side beyond what any budget holds (its product is not formed).  global_only: staged = 0 whatever the size.
static inline int64_t pose_box(const GradGrid &g, const double c[3], double radius, bool global_only, PoseBox *box) {
    int64_t vox = 1;
    for (int k = 0; k < 3; ++k) {
        double first = 0.0, last = 0.0;
        if (!grad_span(g, c, radius, k, &first, &last)) { first = 0.0; last = 0.0; vox = -1; }      // (unreachable after the two checks; kept defined)
        box->lo[k] = (int32_t)first - POSE_GROW;
        box->n[k] = (int32_t)(last - first) + 1 + 2 * POSE_GROW;
        if (box->n[k] > POSE_LDS_BUDGET / 4) vox = -1;
        if (vox >= 0) vox *= box->n[k];
    }
    box->staged = (!global_only && vox >= 0 && pose_lds_bytes(vox) <= POSE_LDS_BUDGET) ? 1 : 0;
    box->pad = 0;
    return vox;
}

// The centres of one launch: as many as keep the score table within POSE_TABLE_BYTES, one at the least.
static inline int64_t pose_chunk(int64_t n_centres, int64_t n_rot) {
    const int64_t fit = POSE_TABLE_BYTES / (POSE_TABLE_ROW * n_rot);
    return std::max<int64_t>(1, std::min(n_centres, fit));
}

// The call's scratch, laid out by ONE carve (the rule of pdbeda_stage.h): the inputs, a chunk's boxes and centres, its score table and its rows.
struct PoseScratch {
    double *frag = nullptr, *w = nullptr, *rot = nullptr, *centres = nullptr;
    PoseBox *box = nullptr;
    double *score = nullptr, *best_score = nullptr;
    int32_t *low = nullptr, *best_rot = nullptr, *best_low = nullptr, *n_kept = nullptr;
    uint8_t *kept = nullptr;
    void carve(Carver &cv, int32_t n_frag, int64_t n_rot, int64_t chunk, int32_t top_k) {
        const size_t nf = (size_t)n_frag, nr = (size_t)n_rot, ch = (size_t)chunk, k = (size_t)top_k;
        cv.take(frag, 3 * nf);
        cv.take(w, nf);
        cv.take(rot, 9 * nr);
        cv.take(centres, 3 * ch);
        cv.take(box, ch);
        cv.take(score, ch * nr);
        cv.take(low, ch * nr);
        cv.take(kept, ch * nr);
        cv.take(best_rot, ch * k);
        cv.take(best_score, ch * k);
        cv.take(best_low, ch * k);
        cv.take(n_kept, ch);
    }
};
static inline size_t pose_scratch_bytes(int32_t n_frag, int64_t n_rot, int64_t chunk, int32_t top_k) {
    Carver size(nullptr);
    PoseScratch s;
    s.carve(size, n_frag, n_rot, chunk, top_k);
    return size.off;
}

}  // namespace pdbeda
