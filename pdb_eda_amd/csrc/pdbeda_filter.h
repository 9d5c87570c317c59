// pdbeda_filter.h -- a resident map through a neighbourhood into a resident map: the separable filter of pdbeda_map_filter and the windowed
// moments of pdbeda_map_local_stats.  No reference counterpart; the contracts are spelled out at those two entry points in
// include/pdbeda.h.  Included from pdbeda_hip.hip.
//
//   k_filter_c<NCH>          the pass along c, and the only one that reads float32 maps.  A workgroup of 256 = FC_RUN lanes along c x FC_ROWS rows
//                            (a row = one (r, s)); every wave stages its row's run plus the 2R halo in LDS through the wrap rule (the other end of
//                            the row, a copy of the cell, or 0.0 for an absent index), then each lane sums its 2R + 1 taps from LDS.  NCH = 1: the
//                            channel a; 2: a, a a; 5: a, a a, b, b b, a b -- the maps are read ONCE and every channel written (the products are
//                            formed in fp64 from float32 values: exact).
//   k_filter_line<OUT>       a pass along r or s over fp64 volumes.  A workgroup of 256 = FL_LANES lanes along c x 8 groups takes FL_CHUNK outputs
//                            of the filtered axis: the FL_CHUNK + 2R input rows (each a coalesced segment of FL_LANES doubles, through the wrap
//                            rule) go to LDS, every thread then owns FL_CHUNK / 8 consecutive outputs of its column and walks the window once, so
//                            a value read from LDS feeds up to four sums.  OUT = double: an unrounded intermediate; OUT = float: the closing pass
//                            of pdbeda_map_filter, with the division by N under PDBEDA_FILTER_RENORMALIZE, rounded once.
//   k_local_finish           voxel-wise: the channels, the maps and the three W arrays into the requested float32 outputs.
//
// The taps travel as a kernel argument (FilterTaps by value, 1 KB): the loop over k is uniform, so they are read by scalar loads into SGPRs.
// Every sum starts at +0.0 and runs over ascending k with a product and a sum rounded separately (-ffp-contract=off); a lane owns its output: no
// atomic, no reduction across lanes, nothing that depends on scheduling.
#pragma once
#include "pdbeda_device.h"

namespace pdbeda {

static constexpr int FC_RUN = 64;                        // outputs along c of one wave of k_filter_c
static constexpr int FC_ROWS = 4;                        // rows of one workgroup of k_filter_c
static constexpr int FL_LANES = 32;                      // columns (along c) of one workgroup of k_filter_line
static constexpr int FL_CHUNK = 32;                      // outputs along the filtered axis of one workgroup of k_filter_line
static constexpr int FL_PER = FL_CHUNK / 8;              // consecutive outputs of one thread
static constexpr int FILTER_MAX_R = PDBEDA_FILTER_MAX_RADIUS;

struct FilterTaps {
    double w[2 * FILTER_MAX_R + 1];
    int32_t radius;
};

// blocks: ceil(nc / FC_RUN) * ceil(rows / FC_ROWS), run fastest.  out: NCH volumes of n_vox doubles, `vol_stride` apart.
template <int NCH>
__global__ void __launch_bounds__(256) k_filter_c(const float *__restrict__ a, const float *__restrict__ b, int nc, int interval, int64_t rows, int runs,
                                                  FilterTaps t, double *__restrict__ out, int64_t vol_stride) {
    __shared__ float s_a[FC_ROWS][FC_RUN + 2 * FILTER_MAX_R];
    __shared__ float s_b[NCH == 5 ? FC_ROWS : 1][FC_RUN + 2 * FILTER_MAX_R];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int R = t.radius;
    const int64_t blk = blockIdx.x;
    const int c0 = (int)(blk % runs) * FC_RUN;
    const int64_t row = (blk / runs) * FC_ROWS + w;
    const bool row_live = row < rows;
    if (row_live) {
        const float *pa = a + row * nc;
        const float *pb = NCH == 5 ? b + row * nc : nullptr;
        for (int j = lane; j < FC_RUN + 2 * R; j += 64) {
            const int src = wrap_axis(c0 - R + j, nc, interval);
            s_a[w][j] = src >= 0 ? pa[src] : 0.0f;
            if (NCH == 5) s_b[w][j] = src >= 0 ? pb[src] : 0.0f;
        }
    }
    __syncthreads();
    const int c = c0 + lane;
    if (!row_live || c >= nc) return;
    double acc[NCH];
    for (int q = 0; q < NCH; ++q) acc[q] = 0.0;
    for (int k = 0; k <= 2 * R; ++k) {
        const double wk = t.w[k];
        const double x = (double)s_a[w][lane + k];
        acc[0] += wk * x;
        if (NCH >= 2) acc[1] += wk * (x * x);
        if (NCH == 5) {
            const double y = (double)s_b[w][lane + k];
            acc[2] += wk * y;
            acc[3] += wk * (y * y);
            acc[4] += wk * (x * y);
        }
    }
    const int64_t at = row * nc + c;
    for (int q = 0; q < NCH; ++q) out[q * vol_stride + at] = acc[q];
}

// One pass along the axis with `n` stored indices, `interval` and element stride `stride`; `n_other` lines per column along the third axis with element
// stride `other_stride`.  blocks: ceil(nc / FL_LANES) * ceil(n / FL_CHUNK) * n_other, columns fastest, then chunks.  Dynamic LDS: (FL_CHUNK + 2R) *
// FL_LANES doubles.  OUT = float: w_c / w_f / w_o (the W arrays along c, the filtered axis and the other axis; null without renormalisation) and
// `f_first` (the filtered axis comes before the other one in crs order: N = (W_c W_r) W_s either way round).
template <typename OUT>
__global__ void __launch_bounds__(256) k_filter_line(const double *__restrict__ in, int nc, int n, int interval, int64_t stride, int n_other, int64_t other_stride,
                                                     int col_tiles, int chunks, FilterTaps t, OUT *__restrict__ out, const double *__restrict__ w_c,
                                                     const double *__restrict__ w_f, const double *__restrict__ w_o, int f_first) {
    extern __shared__ double s_win[];                    // [FL_CHUNK + 2R][FL_LANES]
    const int tx = threadIdx.x & (FL_LANES - 1), ty = threadIdx.x / FL_LANES;
    const int R = t.radius;
    int64_t blk = blockIdx.x;
    const int c = (int)(blk % col_tiles) * FL_LANES + tx;
    blk /= col_tiles;
    const int i0 = (int)(blk % chunks) * FL_CHUNK;
    const int64_t o = blk / chunks;
    if (o >= n_other) return;                            // (never: the grid is exact; uniform)
    const bool col_live = c < nc;
    const double *base = in + o * other_stride + c;
    for (int j = ty; j < FL_CHUNK + 2 * R; j += 8) {
        const int src = wrap_axis(i0 - R + j, n, interval);
        s_win[j * FL_LANES + tx] = (col_live && src >= 0) ? base[(int64_t)src * stride] : 0.0;
    }
    __syncthreads();
    if (!col_live) return;
    double acc[FL_PER];
    for (int q = 0; q < FL_PER; ++q) acc[q] = 0.0;
    const int j0 = ty * FL_PER;                          // the thread's outputs: i0 + j0 + q; output q reads window rows j0 + q + k
    for (int j = 0; j < 2 * R + FL_PER; ++j) {
        const double v = s_win[(j0 + j) * FL_LANES + tx];
#pragma unroll
        for (int q = 0; q < FL_PER; ++q) {
            const int k = j - q;
            if (k >= 0 && k <= 2 * R) acc[q] += t.w[k] * v;
        }
    }
    for (int q = 0; q < FL_PER; ++q) {
        const int i = i0 + j0 + q;
        if (i >= n) break;
        const int64_t at = o * other_stride + (int64_t)i * stride + c;
        if constexpr (sizeof(OUT) == sizeof(double)) {
            out[at] = acc[q];
        } else {
            double v = acc[q];
            if (w_c) {
                const double wf = w_f[i], wo = w_o[o];
                const double N = f_first ? (w_c[c] * wf) * wo : (w_c[c] * wo) * wf;
                v = N > 0.0 ? v / N : 0.0;
            }
            out[at] = (float)v;
        }
    }
}

struct LocalFinishArgs {
    const float *a, *b;                                  // b null: one map
    const double *ch;                                    // F[a], F[a a] (, F[b], F[b b], F[a b]), `vol_stride` apart
    int64_t vol_stride, n_vox;
    int nc, nr;
    const double *w_c, *w_r, *w_s;
    double std_floor;
    float *mean_a, *std_a, *z_a, *mean_b, *std_b, *cc;   // any may be null
};

__device__ inline double clamp_unit(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }      // (a NaN stays a NaN)

__global__ void __launch_bounds__(256) k_local_finish(LocalFinishArgs p) {
    for (int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x; at < p.n_vox; at += (int64_t)gridDim.x * 256) {
        const int64_t row = at / p.nc;
        const int c = (int)(at - row * p.nc);
        const int64_t s = row / p.nr;
        const int r = (int)(row - s * p.nr);
        const double N = (p.w_c[c] * p.w_r[r]) * p.w_s[s];
        const bool ok = N > 0.0;
        double Ea = 0.0, sa = 0.0, za = 0.0, Eb = 0.0, sb = 0.0, cc = 0.0;
        if (ok) {
            Ea = p.ch[at] / N;
            const double Eaa = p.ch[p.vol_stride + at] / N;
            const double ta = Eaa - Ea * Ea;
            const double va = ta > 0.0 ? ta : 0.0;
            sa = __dsqrt_rn(va);
            const double da = sa > p.std_floor ? sa : p.std_floor;
            za = da > 0.0 ? ((double)p.a[at] - Ea) / da : 0.0;
            if (p.b) {
                Eb = p.ch[2 * p.vol_stride + at] / N;
                const double Ebb = p.ch[3 * p.vol_stride + at] / N;
                const double tb = Ebb - Eb * Eb;
                const double vb = tb > 0.0 ? tb : 0.0;
                sb = __dsqrt_rn(vb);
                const double cov = p.ch[4 * p.vol_stride + at] / N - Ea * Eb;
                cc = (va > 0.0 && vb > 0.0) ? clamp_unit(cov / __dsqrt_rn(va * vb)) : 0.0;
            }
        }
        if (p.mean_a) p.mean_a[at] = (float)Ea;
        if (p.std_a) p.std_a[at] = (float)sa;
        if (p.z_a) p.z_a[at] = (float)za;
        if (p.mean_b) p.mean_b[at] = (float)Eb;
        if (p.std_b) p.std_b[at] = (float)sb;
        if (p.cc) p.cc[at] = (float)cc;
    }
}

}  // namespace pdbeda
