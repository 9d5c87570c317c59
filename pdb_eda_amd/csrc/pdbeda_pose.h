// pdbeda_pose.h -- what fits in a blob: a small rigid fragment tried under many rotations at many centres, every pose scored by the map read between
// voxels at its atoms, and the best poses of every centre ranked.  No reference counterpart; the contract is spelled out at pdbeda_pose_scores in
// include/pdbeda.h, the host's plan (checks, the box of a centre, staged or global, the chunks, the scratch) in pdbeda_poseplan.h.  Included from
// pdbeda_hip.hip.
//
//   k_pose_scores        a workgroup of 256 per centre.
//                        Staging: the centre's box (PoseBox, from the host; raw indices, not clipped) is copied into dynamic LDS through fetch_wrapped --
//                        the stored floats, then a stored BIT per voxel (a ballot per 64), the layout and the functor of k_map_resample
//                        (ResampleStaged) -- when the plan marked it staged; all poses of the centre read it from there.  A centre whose box
//                        exceeds POSE_LDS_BUDGET, and a lane whose eight corners are not all inside the box (a rotation that is not orthonormal),
//                        read the map directly (ResampleDirect): the same floats, the same flags, the same arithmetic, the same bytes out.
//                        Scoring: the lanes stride the rotations and a lane owns its pose from the first atom to the last.  The nine rotation
//                        entries are loaded into registers once per pose; the fragment's coordinates and weights are indexed by the wave-uniform
//                        atom counter only, so they come through scalar loads.  A position is c + R x with matvec3's fused dot product and ONE
//                        unfused add; the sample is interp_trilinear_through, pdbeda_interp_density's; the score adds w * v in atom order, product
//                        and sum rounded separately (the library is built with -ffp-contract=off).
//                        Ranking: top_k rounds.  In a round every thread finds, among ITS OWN poses (the ones it wrote: no thread reads another's
//                        rows), the best kept pose that comes strictly after the previous round's winner in the contract's total order (score
//                        descending as numbers, then rotation index ascending); a butterfly over the wave and four LDS slots over the workgroup
//                        pick the winner under the same order.  The order is total, so the winner does not depend on how the fold pairs the lanes.
//
// No floating-point atomic, no sum across lanes: a score depends on the pose and the map alone -- two calls agree to the bit, and the device equals the
// numpy restatement in tests/pose_checker.py to the bit.
#pragma once
#include "pdbeda_poseplan.h"
#include "pdbeda_resample.h"
#include "pdbeda_wave.h"

namespace pdbeda {

struct PoseArgs {
    const Geom *geom;
    const float *dens;
    const double *frag;                  // [n_frag][3]
    const double *w;                     // [n_frag]
    const double *rot;                   // [n_rot][9]
    const double *centres;               // [centres of the launch][3]
    const PoseBox *box;                  // [centres of the launch]
    int n_frag, n_rot, top_k;
    double floor_d;                      // (double)floor of the call
    int max_low, allow_outside;
    double *score;                       // [centres][n_rot]
    int32_t *low;                        // [centres][n_rot]
    uint8_t *kept;                       // [centres][n_rot]
    int32_t *best_rot;                   // [centres][top_k]
    double *best_score;                  // [centres][top_k]
    int32_t *best_low;                   // [centres][top_k]
    int32_t *n_kept;                     // [centres]
};

// Pose (s1, i1) comes before pose (s2, i2); an index of -1 is "no pose" and comes after every pose.
__device__ __forceinline__ bool pose_before(double s1, int i1, double s2, int i2) {
    return i1 >= 0 && (i2 < 0 || s1 > s2 || (s1 == s2 && i1 < i2));
}

__global__ void __launch_bounds__(256) k_pose_scores(PoseArgs a) {
    extern __shared__ unsigned long long s_pose[];      // the box's stored bits [words], then its floats [n_box]
    __shared__ double s_best[4];
    __shared__ int s_index[4], s_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Geom &g = *a.geom;
    const int64_t centre = blockIdx.x;
    const PoseBox b = a.box[centre];      // (the same record in every lane: one decision for the workgroup)
    const double c[3] = {a.centres[3 * centre], a.centres[3 * centre + 1], a.centres[3 * centre + 2]};
    const int n_box = b.staged ? b.n[0] * b.n[1] * b.n[2] : 0;
    float *s_val = reinterpret_cast<float *>(s_pose + (n_box + 63) / 64);
    if (b.staged) {
        for (int i0 = wv * 64; i0 < n_box; i0 += 256) {      // (wave-uniform bounds: the ballot sees whole waves)
            const int i = i0 + lane;
            bool ok = false;
            if (i < n_box) {
                const int row = i / b.n[0], dc = i - row * b.n[0], ds = row / b.n[1], dr = row - ds * b.n[1];
                s_val[i] = fetch_wrapped(g, a.dens, b.lo[0] + dc, b.lo[1] + dr, b.lo[2] + ds, &ok);
            }
            const unsigned long long m = __ballot(ok);
            if (lane == 0) s_pose[i0 >> 6] = m;
        }
        __syncthreads();      // (the box is only read from here on)
    }
    const ResampleStaged staged = {s_val, s_pose, {b.lo[0], b.lo[1], b.lo[2]}, b.n[0], b.n[1]};
    const ResampleDirect direct = {g, a.dens};
    double *score = a.score + centre * a.n_rot;
    int32_t *low = a.low + centre * a.n_rot;
    uint8_t *kept = a.kept + centre * a.n_rot;

    int count = 0;
    for (int r = tid; r < a.n_rot; r += 256) {
        double R[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = a.rot[9 * (int64_t)r + j];
        double s = 0.0;
        int n_low = 0;
        bool all_valid = true;
        for (int at = 0; at < a.n_frag; ++at) {      // (wave-uniform: the fragment comes through scalar loads)
            const double x0 = a.frag[3 * at], x1 = a.frag[3 * at + 1], x2 = a.frag[3 * at + 2], w = a.w[at];
            double p[3], f[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = c[i] + fma(R[3 * i + 2], x2, fma(R[3 * i], x0, R[3 * i + 1] * x1));
            xyz2frac(g, p, f);
            bool sane = true, inside = b.staged != 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                sane = sane && fabs(f[q]) < 0x1p29;      // (a NaN fails: a rotation that is no rotation can send an atom anywhere)
                const int first = (int)floor(sane ? f[q] : 0.0) - b.lo[q];
                inside = inside && first >= 0 && first + 1 < b.n[q];
            }
            double v = NAN;
            bool ok = false;
            if (sane) v = inside ? interp_trilinear_through(staged, f, &ok) : interp_trilinear_through(direct, f, &ok);
            s = s + w * v;
            n_low += v < a.floor_d ? 1 : 0;
            all_valid = all_valid && ok;
        }
        const bool keep = !(n_low > a.max_low) && !isnan(s) && (all_valid || a.allow_outside);
        score[r] = isnan(s) ? (double)NAN : s;      // (one NaN for all: which operand's payload survives a sum is the compiler's choice, and differs between the two fetches)
        low[r] = n_low;
        kept[r] = keep ? 1 : 0;
        count += keep ? 1 : 0;
    }
    count = wave_fold<SegAdd>(count);
    if (lane == 0) s_count[wv] = count;

    // the ranking: round k finds the pose that comes next after (prev_s, prev_i); every thread walks the rows it wrote itself
    double prev_s = 0.0;
    int prev_i = -1, filled = 0;
    for (; filled < a.top_k; ++filled) {
        double bs = 0.0;
        int bi = -1;
        for (int r = tid; r < a.n_rot; r += 256) {
            if (!kept[r]) continue;
            const double s = score[r];
            const bool after = prev_i < 0 || s < prev_s || (s == prev_s && r > prev_i);
            if (after && pose_before(s, r, bs, bi)) { bs = s; bi = r; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(bs, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (pose_before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { s_best[wv] = bs; s_index[wv] = bi; }
        __syncthreads();
        bs = s_best[0]; bi = s_index[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (pose_before(s_best[k], s_index[k], bs, bi)) { bs = s_best[k]; bi = s_index[k]; }
        __syncthreads();      // (the slots are read: the next round may write them)
        if (bi < 0) break;      // (the same in every thread: the kept poses are used up)
        if (tid == 0) {
            a.best_rot[centre * a.top_k + filled] = bi;
            a.best_score[centre * a.top_k + filled] = bs;
        }
        if (bi % 256 == tid) a.best_low[centre * a.top_k + filled] = low[bi];      // (the thread that wrote the row reads it)
        prev_s = bs; prev_i = bi;
    }
    if (tid == 0) {
        for (int k = filled; k < a.top_k; ++k) {
            a.best_rot[centre * a.top_k + k] = -1;
            a.best_score[centre * a.top_k + k] = 0.0;
            a.best_low[centre * a.top_k + k] = 0;
        }
        a.n_kept[centre] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);      // (the first round's barrier stands between the writes and this read)
    }
}

}  // namespace pdbeda
