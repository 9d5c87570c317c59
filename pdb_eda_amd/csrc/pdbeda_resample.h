// pdbeda_resample.h -- a map carried to ANOTHER grid through coordinate operators: for every voxel of a destination grid, pull its position back
// through one or more affine operators into the source map and interpolate there (nearest, trilinear, Catmull-Rom tricubic).  No reference
// counterpart; the contract is spelled out at pdbeda_map_resample in include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   resample_sample      one sample at a fractional grid position through a fetch functor: the taps an axis USES are b (t == 0), b and b + 1
//                        (order 1) or b - 1 .. b + 2 (order 3); folded along c, then r, then s in unfused fp64.  Valid: every used tap is stored.
//   k_map_resample       a workgroup of 256 per destination tile of RS_C x RS_R x RS_S voxels (rows of 128 bytes along c), one thread per voxel.
//                        Per operator (read through wave-uniform addresses) the tile's eight corners -- one per lane, folded by shuffles -- give a box of source indices; grown by the
//                        support and one voxel of safety it is staged in LDS through fetch_wrapped when it holds at most RS_LDS_VOX voxels --
//                        values plus a stored BIT per voxel (a ballot per 64) -- and every tap of the tile then comes from LDS: at order 3,
//                        where a voxel has 64 taps; at orders 0 and 1 every tap is a direct load (measured: DESIGN.md 4.15).  A box beyond
//                        the budget, and a lane whose support is not wholly inside the staged box, read the map directly: the two fetches
//                        return the same floats and the same stored flags, so no result depends on the box.  In first-valid mode the
//                        workgroup leaves the operator loop when all its voxels are served.
//
// A lane owns its voxel: no floating-point atomic, no reduction across lanes, the operators in index order -- two calls agree to the bit, and
// the device equals the numpy restatement in tests/resample_checker.py.
#pragma once
#include "pdbeda_qscore.h"

namespace pdbeda {

static constexpr int RS_C = 32, RS_R = 4, RS_S = 2;      // the destination tile: 256 voxels, c fastest
static constexpr int RS_LDS_VOX = 8192;                  // source voxels a workgroup stages at the most: 32 KB of values + 1 KB of stored bits
static constexpr int RS_CTR_SLOTS = 256;                 // rows of four counters the workgroups spread their integer atomics over

struct ResampleArgs {
    const Geom *src_geom;
    const float *src;
    const Geom *dst_geom;
    int tiles_c, tiles_r;                // tiles along c and r (tile number = (ts * tiles_r + tr) * tiles_c + tc)
    const double *ops;                   // [n_ops][12], rows of [R | t]
    int n_ops;
    int mean;                            // PDBEDA_RESAMPLE_MEAN
    int stage;                           // 0: direct loads only; 1: staged boxes; 2: staged boxes that are NOT grown (lanes at the rim leave them: a test's hook)
    float fill;
    const float *base;                   // [dst voxels], or nullptr
    double alpha;
    float *out;                          // [dst voxels]
    float *coverage;                     // [dst voxels], or nullptr
    unsigned long long *counters;        // [RS_CTR_SLOTS][4]: voxels with count > 0, with count 0, (tile, operator) pairs staged, pairs read directly
};

struct ResampleDirect {
    const Geom &g;
    const float *__restrict__ dens;
    __device__ float operator()(int c, int r, int s, bool *ok) const { return fetch_wrapped(g, dens, c, r, s, ok); }
};
struct ResampleStaged {
    const float *val;
    const unsigned long long *bits;
    int lo[3], dc, dr;
    __device__ float operator()(int c, int r, int s, bool *ok) const {
        const int i = ((s - lo[2]) * dr + (r - lo[1])) * dc + (c - lo[0]);
        *ok = (bits[i >> 6] >> (i & 63)) & 1ull;
        return val[i];
    }
};

// x = R p + t with symmetry_candidate's arithmetic.
__host__ __device__ inline void resample_apply(const double *__restrict__ op, const double p[3], double x[3]) {
    for (int i = 0; i < 3; ++i) x[i] = ((op[4 * i] * p[0] + op[4 * i + 1] * p[1]) + op[4 * i + 2] * p[2]) + op[4 * i + 3];
}

// The first and the last index an order may touch relative to floor(f) (order 0: relative to rint(f)).
template <int ORDER> struct ResampleSupport { static constexpr int lo = ORDER == 3 ? -1 : 0, hi = ORDER == 3 ? 2 : (ORDER == 1 ? 1 : 0); };

// One axis of the fold: N taps v, of which only v[K0] counts when t == 0.
template <int ORDER>
__device__ inline double resample_fold(const double v[4], double t, const double w[4]) {
    constexpr int K0 = ORDER == 3 ? 1 : 0;
    if (t == 0.0) return v[K0];
    if (ORDER == 1) return v[0] + t * (v[1] - v[0]);
    return ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3];
}

template <int ORDER, typename Fetch>
__device__ inline double resample_sample(const double f[3], const Fetch &fetch, bool *valid) {
    if (ORDER == 0) {
        bool ok;
        const double v = (double)fetch((int32_t)rint(f[0]), (int32_t)rint(f[1]), (int32_t)rint(f[2]), &ok);
        *valid = ok;
        return v;
    }
    constexpr int N = ORDER == 3 ? 4 : 2, K0 = ORDER == 3 ? 1 : 0;
    int32_t b[3];
    double t[3], w[3][4];
    for (int q = 0; q < 3; ++q) {
        const double fl = floor(f[q]);
        b[q] = (int32_t)fl - K0;      // the first tap's index
        t[q] = f[q] - fl;
        const double u = t[q];
        w[q][0] = ((-0.5 * u + 1.0) * u - 0.5) * u;
        w[q][1] = ((1.5 * u - 2.5) * u) * u + 1.0;
        w[q][2] = ((-1.5 * u + 2.0) * u + 0.5) * u;
        w[q][3] = ((0.5 * u - 0.5) * u) * u;
    }
    bool all = true;
    double ys[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < N; ++ks) {
        if (t[2] == 0.0 && ks != K0) continue;
        double yr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kr = 0; kr < N; ++kr) {
            if (t[1] == 0.0 && kr != K0) continue;
            double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kc = 0; kc < N; ++kc) {
                if (t[0] == 0.0 && kc != K0) continue;
                bool ok;
                v[kc] = (double)fetch(b[0] + kc, b[1] + kr, b[2] + ks, &ok);
                all = all && ok;
            }
            yr[kr] = resample_fold<ORDER>(v, t[0], w[0]);
        }
        ys[ks] = resample_fold<ORDER>(yr, t[1], w[1]);
    }
    *valid = all;
    return resample_fold<ORDER>(ys, t[2], w[2]);
}

template <int ORDER>
__global__ void __launch_bounds__(256) k_map_resample(ResampleArgs a) {
    __shared__ float s_val[RS_LDS_VOX];
    __shared__ unsigned long long s_bits[RS_LDS_VOX / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Geom &gs = *a.src_geom;
    const Geom &gd = *a.dst_geom;
    const TileVoxel tv = tile_voxel<RS_C, RS_R, RS_S>(blockIdx.x, a.tiles_c, a.tiles_r, gd.ncrs, tid);
    const bool live = tv.live;
    double p[3] = {0.0, 0.0, 0.0};
    if (live) crs2xyz(gd, tv.c, tv.r, tv.s, p);
    double corner[3];      // lane l holds corner l & 7 of the tile, in destination coordinates: a group of eight lanes holds them all
    crs2xyz(gd, (lane & 1) ? tv.c1[0] : tv.c0[0], (lane & 2) ? tv.c1[1] : tv.c0[1], (lane & 4) ? tv.c1[2] : tv.c0[2], corner);
    const ResampleDirect direct = {gs, a.src};
    constexpr int grow_lo = 1 - ResampleSupport<ORDER>::lo, grow_hi = 1 + ResampleSupport<ORDER>::hi;      // the support and one voxel of safety

    int count = 0;
    double value = 0.0;
    unsigned n_staged = 0, n_direct = 0;
    for (int k = 0; k < a.n_ops; ++k) {
        const double *__restrict__ op = a.ops + 12 * k;
        // the box of source indices under this operator: the same numbers in every lane, hence one decision for the workgroup
        ResampleStaged staged = {s_val, s_bits, {0, 0, 0}, 0, 0};
        int dim[3] = {0, 0, 0};
        bool use_lds = false;
        if (a.stage && ORDER == 3) {      // (measured: at orders 0 and 1 a voxel's one to eight taps do not repay the staging pass)
            double mn[3], mx[3];
            {
                double x[3], f[3];
                resample_apply(op, corner, x);
                xyz2frac(gs, x, f);
                for (int q = 0; q < 3; ++q) {      // min and max over the eight corners: a butterfly inside every group of eight lanes, the same in all of them
                    mn[q] = mx[q] = f[q];
                    for (int off = 1; off < 8; off <<= 1) { mn[q] = fmin(mn[q], __shfl_xor(mn[q], off, 64)); mx[q] = fmax(mx[q], __shfl_xor(mx[q], off, 64)); }
                }
            }
            const int grow[2] = {a.stage == 2 ? 0 : grow_lo, a.stage == 2 ? 0 : grow_hi};
            bool fits = true;
            for (int q = 0; q < 3; ++q) {
                const bool sane = fabs(mn[q]) < 0x1p29 && fabs(mx[q]) < 0x1p29;      // (the host has checked it; a NaN fails here)
                const int32_t lo = (int32_t)floor(sane ? mn[q] : 0.0) - grow[0], hi = (int32_t)ceil(sane ? mx[q] : 0.0) + grow[1];
                fits = fits && sane && hi - lo < RS_LDS_VOX;
                staged.lo[q] = lo;
                dim[q] = fits ? hi - lo + 1 : 0;
            }
            use_lds = fits && (int64_t)dim[0] * dim[1] * dim[2] <= RS_LDS_VOX;
            staged.dc = dim[0]; staged.dr = dim[1];
            if (use_lds) {
                const int n_box = dim[0] * dim[1] * dim[2];
                __syncthreads();      // (the last operator's taps are read)
                for (int i0 = wv * 64; i0 < n_box; i0 += 256) {      // (wave-uniform bounds: the ballot sees whole waves)
                    const int i = i0 + lane;
                    bool ok = false;
                    if (i < n_box) {
                        const int row = i / dim[0], c = i - row * dim[0], s = row / dim[1], r = row - s * dim[1];
                        s_val[i] = fetch_wrapped(gs, a.src, staged.lo[0] + c, staged.lo[1] + r, staged.lo[2] + s, &ok);
                    }
                    const unsigned long long m = __ballot(ok);
                    if (lane == 0) s_bits[i0 >> 6] = m;
                }
                __syncthreads();
            }
        }
        if (use_lds) ++n_staged; else ++n_direct;

        if (live && (a.mean || count == 0)) {
            double x[3], f[3];
            resample_apply(op, p, x);
            xyz2frac(gs, x, f);
            bool inside = use_lds;      // this sample's whole support lies in the staged box
            for (int q = 0; q < 3; ++q) {
                const double rn = rint(f[q]);
                if (fabs(f[q] - rn) <= 0x1p-26) f[q] = rn;
                const int64_t first = (int64_t)(ORDER == 0 ? rn : floor(f[q])) + ResampleSupport<ORDER>::lo - staged.lo[q];
                inside = inside && first >= 0 && first + (ResampleSupport<ORDER>::hi - ResampleSupport<ORDER>::lo) < dim[q];
            }
            bool ok;
            const double v = inside ? resample_sample<ORDER>(f, staged, &ok) : resample_sample<ORDER>(f, direct, &ok);
            if (ok) {
                value = a.mean ? value + v : v;
                ++count;
            }
        }
        if (!a.mean && __syncthreads_and(!live || count > 0)) break;
    }

    if (live) {
        const int64_t at = ((int64_t)tv.s * gd.ncrs[1] + tv.r) * gd.ncrs[0] + tv.c;
        float res = a.fill;
        if (count > 0) {
            const double val = a.mean ? value / (double)count : value;
            res = a.base ? (float)((double)a.base[at] + a.alpha * val) : (float)val;
        }
        a.out[at] = res;
        if (a.coverage) a.coverage[at] = (float)count;
    }
    // the counters: one row of RS_CTR_SLOTS per workgroup residue, so that 2^16 workgroups do not queue up on four addresses (the host adds the rows)
    const int n_hit = __syncthreads_count(live && count > 0);
    if (tid == 0) {
        unsigned long long *row = a.counters + 4 * (blockIdx.x % RS_CTR_SLOTS);
        const int n_live = (tv.c1[0] - tv.c0[0] + 1) * (tv.c1[1] - tv.c0[1] + 1) * (tv.c1[2] - tv.c0[2] + 1);
        if (n_hit) atomicAdd(&row[0], (unsigned long long)n_hit);
        if (n_live - n_hit) atomicAdd(&row[1], (unsigned long long)(n_live - n_hit));
        if (n_staged) atomicAdd(&row[2], (unsigned long long)n_staged);
        if (n_direct) atomicAdd(&row[3], (unsigned long long)n_direct);
    }
}

}  // namespace pdbeda
