// pdbeda_fourier.h -- reciprocal space: the 3-D transform of a resident map into its Hermitian half spectrum and back, and what works on a resident
// spectrum (radial scaling, shell sums, single coefficients).  No reference counterpart; the contracts are spelled out at pdbeda_map_fft,
// pdbeda_spectrum_inverse, pdbeda_spectrum_scale, pdbeda_spectrum_shells and pdbeda_spectrum_values in include/pdbeda.h.  Included from pdbeda_hip.hip.
// The arithmetic of a line is pdbeda_fourier_line.h's butterfly, the same code the host runs; device code computes no sine or cosine.
//
// A spectrum is [ns][nr][nh] complex fp64, nh = nc / 2 + 1.  Every transform kernel is a workgroup of 256 over a TILE of FFT_LINES = 4 lines of one
// length n, interleaved in LDS as [i][line] (element i of the four lines in 64 consecutive bytes): two such buffers for the autosort passes and the
// line's twiddle table, 144 n bytes -- 144 KiB at n = 1024.  The kernels are instantiated for NMAX = 64, 128, 256, 512, 1024 (static LDS of
// 144 NMAX bytes; the host takes the smallest NMAX >= n), so a 256-long line leaves room for four workgroups on a CU.  In a pass the 4 (n / r)
// butterflies of the tile go round the lanes, line fastest: the four lanes of a butterfly index read 64 consecutive bytes, and consecutive butterflies
// read consecutive addresses (the input index of butterfly t is t + k s m), so the reads have no bank conflict; the writes of the FIRST pass (s = 1)
// are 64-byte pieces 64 r bytes apart, a conflict of up to r ways on the 64-bank LDS, and contiguous runs of s pieces from the second pass on.
//
//   k_fft_rows<NMAX>      forward along c: FFT_ROWS = 4 rows (a row = one (r, s)) of float32, widened to (x, 0) in LDS, run as complex lines of nc with
//                         zero imaginary part (no two-rows-in-one or half-length trick: the defined bits are those of the plain complex line), columns
//                         0 .. nc / 2 stored.  A lane loads one column of the four rows (four coalesced 4-byte loads, one 64-byte LDS store).
//   k_fft_cols<NMAX>      along r or s, either direction: FFT_COLS = 4 adjacent half-spectrum columns times the whole line; every global load and store
//                         of a line group is 64 contiguous bytes.  Columns past nh in the last tile are zero lines that are not stored.  A workgroup
//                         reads all of its lines before it writes any, so the pass may run in place.
//   k_ifft_rows<NMAX>     inverse along c: the half row is mirrored into the whole Hermitian line in LDS (the imaginary parts of column 0 and, for even
//                         nc, of column nc / 2 are dropped), the line runs, and voxel = float32(re / (double)N).
//   k_spectrum_scale      coefficient-wise, the table in LDS.
//   k_spectrum_shells     per-workgroup per-shell partials without atomics: 256 coefficients at a time put (shell, weight, terms) in LDS, then the lanes
//                         of shell j add its entries in index order; k_spectrum_shells_fold folds the workgroups' rows of a shell in a fixed order.
//   k_spectrum_values     single coefficients, the missing half through the Hermitian mirror.
// A lane owns its outputs; there is no atomic anywhere in this file.
#pragma once
#include "pdbeda_device.h"
#include "pdbeda_fourier_line.h"

namespace pdbeda {

static constexpr int FFT_LINES = 4;                      // lines of one tile
static constexpr int FFT_ROWS = FFT_LINES;               // rows of one workgroup of k_fft_rows / k_ifft_rows
static constexpr int FFT_COLS = FFT_LINES;               // half-spectrum columns of one workgroup of k_fft_cols
static constexpr int FFT_SHELL_BLOCKS = 1024;            // the most workgroups of k_spectrum_shells
static constexpr int FFT_MAX_TABLE = PDBEDA_SPECTRUM_MAX_TABLE;
static constexpr int FFT_MAX_SHELLS = PDBEDA_SPECTRUM_MAX_SHELLS;

// The passes of a tile: a -> b -> a ...; returns the buffer that holds the result.  All 256 threads call it.
__device__ inline FftCplx *fft_tile_run(FftCplx *a, FftCplx *b, const FftCplx *w, const FftPlan &plan, int inverse) {
    int s = 1;
    for (int i = 0; i < plan.n_pass; ++i) {
        const int r = plan.radix[i], work = (plan.n / r) * FFT_LINES;
        for (int idx = threadIdx.x; idx < work; idx += 256)
            pdbeda_fft_butterfly(a + (idx & (FFT_LINES - 1)), b + (idx & (FFT_LINES - 1)), FFT_LINES, plan.n, s, r, idx / FFT_LINES, w, inverse);
        __syncthreads();
        FftCplx *z = a; a = b; b = z;
        s *= r;
    }
    return a;
}

// blocks: ceil(rows / FFT_ROWS).  in: [rows][nc] float32; out: [rows][nh].
template <int NMAX>
__global__ void __launch_bounds__(256) k_fft_rows(const float *__restrict__ in, int64_t rows, FftPlan plan, const FftCplx *__restrict__ tw, FftCplx *__restrict__ out) {
    __shared__ FftCplx s_a[NMAX * FFT_LINES], s_b[NMAX * FFT_LINES], s_w[NMAX];
    const int n = plan.n, nh = n / 2 + 1;
    const int64_t row0 = (int64_t)blockIdx.x * FFT_ROWS;
    for (int i = threadIdx.x; i < n; i += 256) {
        s_w[i] = tw[i];
        for (int l = 0; l < FFT_ROWS; ++l) s_a[i * FFT_LINES + l] = FftCplx{row0 + l < rows ? (double)in[(row0 + l) * n + i] : 0.0, 0.0};
    }
    __syncthreads();
    const FftCplx *res = fft_tile_run(s_a, s_b, s_w, plan, 0);
    for (int idx = threadIdx.x; idx < nh * FFT_ROWS; idx += 256) {
        const int l = idx / nh, h = idx - l * nh;
        if (row0 + l < rows) out[(row0 + l) * nh + h] = res[h * FFT_LINES + l];
    }
}

// blocks: ceil(nh / FFT_COLS) * n_other, column tile fastest.  Element i of the line (column h, other index o) is at o * other_stride + i * stride + h.
template <int NMAX>
__global__ void __launch_bounds__(256) k_fft_cols(const FftCplx *in, int nh, int col_tiles, int64_t stride, int64_t other_stride, FftPlan plan, const FftCplx *__restrict__ tw,
                                                  int inverse, FftCplx *out) {
    __shared__ FftCplx s_a[NMAX * FFT_LINES], s_b[NMAX * FFT_LINES], s_w[NMAX];
    const int n = plan.n;
    const int64_t blk = blockIdx.x;
    const int h0 = (int)(blk % col_tiles) * FFT_COLS;
    const int64_t base = (blk / col_tiles) * other_stride + h0;
    for (int i = threadIdx.x; i < n; i += 256) s_w[i] = tw[i];
    for (int idx = threadIdx.x; idx < n * FFT_LINES; idx += 256) {
        const int i = idx / FFT_LINES, l = idx & (FFT_LINES - 1);
        s_a[idx] = h0 + l < nh ? in[base + i * stride + l] : FftCplx{0.0, 0.0};
    }
    __syncthreads();
    const FftCplx *res = fft_tile_run(s_a, s_b, s_w, plan, inverse);
    for (int idx = threadIdx.x; idx < n * FFT_LINES; idx += 256) {
        const int i = idx / FFT_LINES, l = idx & (FFT_LINES - 1);
        if (h0 + l < nh) out[base + i * stride + l] = res[idx];
    }
}

// blocks: ceil(rows / FFT_ROWS).  in: [rows][nh]; out: [rows][nc] float32 = float32(re / n_total).
template <int NMAX>
__global__ void __launch_bounds__(256) k_ifft_rows(const FftCplx *__restrict__ in, int64_t rows, FftPlan plan, const FftCplx *__restrict__ tw, double n_total, float *__restrict__ out) {
    __shared__ FftCplx s_a[NMAX * FFT_LINES], s_b[NMAX * FFT_LINES], s_w[NMAX];
    const int n = plan.n, nh = n / 2 + 1;
    const int64_t row0 = (int64_t)blockIdx.x * FFT_ROWS;
    for (int i = threadIdx.x; i < n; i += 256) s_w[i] = tw[i];
    for (int idx = threadIdx.x; idx < nh * FFT_ROWS; idx += 256) {
        const int l = idx / nh, h = idx - l * nh;
        FftCplx v = row0 + l < rows ? in[(row0 + l) * nh + h] : FftCplx{0.0, 0.0};
        if (h == 0 || 2 * h == n) v.im = 0.0;
        s_a[h * FFT_LINES + l] = v;
        if (h > 0 && 2 * h < n) s_a[(n - h) * FFT_LINES + l] = FftCplx{v.re, -v.im};
    }
    __syncthreads();
    const FftCplx *res = fft_tile_run(s_a, s_b, s_w, plan, 1);
    for (int idx = threadIdx.x; idx < n * FFT_ROWS; idx += 256) {
        const int l = idx / n, i = idx - l * n;
        if (row0 + l < rows) out[(row0 + l) * n + i] = (float)(res[i * FFT_LINES + l].re / n_total);
    }
}

// ---- on a resident spectrum -----------------------------------------------------------------------------------------------------------------
struct SpectrumShape {
    int32_t nc, nr, ns, nh;
    int64_t n_coef;
    double m[6];      // the caller's metric: m00, m11, m22, m01, m02, m12
};

// The frequency number of index j on an axis of n.
__host__ __device__ inline int fft_freq(int j, int n) { return 2 * j <= n ? j : j - n; }

// s^2 of a coefficient, in the contract's order; the integer products are exact.
__host__ __device__ inline double fft_s2(const double m[6], int h0, int h1, int h2) {
    const double d0 = m[0] * (double)(h0 * h0), d1 = m[1] * (double)(h1 * h1), d2 = m[2] * (double)(h2 * h2);
    const double x01 = m[3] * (double)(h0 * h1), x02 = m[4] * (double)(h0 * h2), x12 = m[5] * (double)(h1 * h2);
    return ((d0 + d1) + d2) + 2.0 * ((x01 + x02) + x12);
}

__device__ inline double fft_s2_at(const SpectrumShape &sh, int64_t i, int *col) {
    const int64_t row = i / sh.nh;
    const int h = (int)(i - row * sh.nh);
    const int s = (int)(row / sh.nr), r = (int)(row - (int64_t)s * sh.nr);
    *col = h;
    return fft_s2(sh.m, fft_freq(h, sh.nc), fft_freq(r, sh.nr), fft_freq(s, sh.ns));
}

// t_scale = (n_table - 1) / s2_max, from the host.
__global__ void __launch_bounds__(256) k_spectrum_scale(FftCplx *__restrict__ data, SpectrumShape sh, const double *__restrict__ table, int n_table, double t_scale, double beyond) {
    __shared__ double s_t[FFT_MAX_TABLE];
    for (int k = threadIdx.x; k < n_table; k += 256) s_t[k] = table[k];
    __syncthreads();
    const double last = (double)(n_table - 1);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sh.n_coef; i += (int64_t)gridDim.x * 256) {
        int col;
        const double t = fft_s2_at(sh, i, &col) * t_scale;
        double g;
        if (t > last) g = beyond;
        else if (t == last) g = s_t[n_table - 1];
        else if (!(t >= 0.0)) g = s_t[0];      // (s^2 < 0: a metric that is not positive definite)
        else {
            const double fl = floor(t);
            const int k = (int)fl;
            g = s_t[k] + (t - fl) * (s_t[k + 1] - s_t[k]);
        }
        const FftCplx v = data[i];
        data[i] = FftCplx{v.re * g, v.im * g};
    }
}

// Workgroup w takes the coefficients [w * chunk, (w + 1) * chunk), chunk a multiple of 256, 256 at a time: every lane puts its coefficient's shell, weight
// and terms in LDS; then lane p * n_shells + j (p < parts, parts * n_shells <= 256, parts a power of two from the host) adds the entries of shell j in
// segment p of the 256 in index order, to its own running sums; at the end lane j adds the parts' sums in the order of p.  One order for one shape and one
// n_shells.  partials: [gridDim.x][n_shells][5] -- the count (below 2^53 as a double: exact), sum w |A|^2, sum w |B|^2, sum w Re(A conj B),
// sum w Im(A conj B).  b may be null.
__global__ void __launch_bounds__(256) k_spectrum_shells(const FftCplx *__restrict__ a, const FftCplx *__restrict__ b, SpectrumShape sh, const double *__restrict__ edges, int n_shells,
                                                         int parts, int64_t chunk, double *__restrict__ partials) {
    __shared__ double s_edge[FFT_MAX_SHELLS + 1];
    __shared__ int s_shell[256];
    __shared__ double s_v[5][256];
    for (int k = threadIdx.x; k <= n_shells; k += 256) s_edge[k] = edges[k];
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < sh.n_coef ? lo + chunk : sh.n_coef;
    const int me = threadIdx.x;
    const int seg = 256 / parts, my_part = me / n_shells, my_shell = me - my_part * n_shells;
    const bool scans = my_part < parts;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t i = base + me;
        int shell = -1;
        if (i < hi) {
            int col;
            const double s2 = fft_s2_at(sh, i, &col);
            if (s2 >= s_edge[0] && s2 < s_edge[n_shells]) {
                int l = 0, h = n_shells;      // edges[l] <= s2 < edges[h]
                while (h - l > 1) {
                    const int mid = (l + h) >> 1;
                    if (s2 >= s_edge[mid]) l = mid; else h = mid;
                }
                shell = l;
                const double w = (col == 0 || 2 * col == sh.nc) ? 1.0 : 2.0;
                const FftCplx A = a[i];
                s_v[0][me] = w;
                s_v[1][me] = w * (A.re * A.re + A.im * A.im);
                if (b) {
                    const FftCplx B = b[i];
                    s_v[2][me] = w * (B.re * B.re + B.im * B.im);
                    s_v[3][me] = w * (A.re * B.re + A.im * B.im);
                    s_v[4][me] = w * (A.im * B.re - A.re * B.im);
                } else {
                    s_v[2][me] = 0.0; s_v[3][me] = 0.0; s_v[4][me] = 0.0;
                }
            }
        }
        s_shell[me] = shell;
        __syncthreads();
        if (scans)
            for (int e = my_part * seg; e < (my_part + 1) * seg; ++e)
                if (s_shell[e] == my_shell)
                    for (int k = 0; k < 5; ++k) acc[k] += s_v[k][e];
        __syncthreads();
    }
    for (int k = 0; k < 5; ++k) s_v[k][me] = acc[k];
    __syncthreads();
    if (me < n_shells)
        for (int k = 0; k < 5; ++k) {
            double total = s_v[k][me];
            for (int p = 1; p < parts; ++p) total += s_v[k][p * n_shells + me];
            partials[((size_t)blockIdx.x * n_shells + me) * 5 + k] = total;
        }
}

// Workgroup j folds shell j: thread t adds the rows t, t + 256, ... in this order, then the 256 sums fold as a binary tree (k_pair_moments_fold's order).
// out: [n_shells][5].
__global__ void __launch_bounds__(256) k_spectrum_shells_fold(const double *__restrict__ partials, int n_rows, int n_shells, double *__restrict__ out) {
    __shared__ double s_part[5][256];
    const int j = blockIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int w = threadIdx.x; w < n_rows; w += 256)
        for (int k = 0; k < 5; ++k) v[k] += partials[((size_t)w * n_shells + j) * 5 + k];
    for (int k = 0; k < 5; ++k) s_part[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 5; ++k) s_part[k][threadIdx.x] += s_part[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 5) out[j * 5 + threadIdx.x] = s_part[threadIdx.x][0];
}

// idx: [n][3] in crs order, any integers; out: [n][2].
__global__ void __launch_bounds__(256) k_spectrum_values(const FftCplx *__restrict__ data, SpectrumShape sh, const int32_t *__restrict__ idx, int64_t n, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int c = floor_mod(idx[3 * i], sh.nc), r = floor_mod(idx[3 * i + 1], sh.nr), s = floor_mod(idx[3 * i + 2], sh.ns);
    const bool mirror = c >= sh.nh;
    if (mirror) { c = sh.nc - c; r = r ? sh.nr - r : 0; s = s ? sh.ns - s : 0; }
    const FftCplx v = data[((int64_t)s * sh.nr + r) * sh.nh + c];
    out[2 * i] = v.re;
    out[2 * i + 1] = mirror ? -v.im : v.im;
}

}  // namespace pdbeda
