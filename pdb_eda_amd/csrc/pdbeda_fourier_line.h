// pdbeda_fourier_line.h -- one line of a Fourier transform: the planner, the twiddle table and the butterfly of an autosort (Stockham) mixed-radix
// FFT on complex fp64.  No HIP: a plain C++ compiler reads the file (tests/fourier_harness.cpp builds it under the host's sanitizers), and the kernels
// of pdbeda_fourier.h run the SAME butterfly, so a line has the same bits on the host and on the device, wherever it sits in a tile and whichever
// lane works on it.  Everything is plain IEEE fp64 multiplies and adds (the library is built with -ffp-contract=off) in an order fixed by n and the
// direction.  The contract of the transform: pdbeda_map_fft in include/pdbeda.h.
//
// The plan.  pdbeda_fft_plan(n) is a function of n alone: n = 2^a 3^b 5^c 7^d, 1 <= n <= PDBEDA_FFT_MAX_AXIS; the radix sequence is
//     4 (a / 2 times), 2 (once if a is odd), 3 (b times), 5 (c times), 7 (d times)
// in this order (at most PDBEDA_FFT_MAX_PASSES = 6 radices up to 1024: 2 * 3^5 = 486, 4 * 3^5 = 972 and 3^6 = 729 are the longest).  n = 1 has no pass.
//
// A pass.  With the radices r_1 .. r_P, pass i has s = r_1 .. r_(i-1) (the stride reached so far), m = n / (s r_i), and n / r_i butterflies; butterfly t has
// p = t / s, q = t % s, reads a_k = x[q + s (p + k m)], k = 0 .. r - 1, and writes
//     y[q + s (r p + j)] = (sum_k a_k w_r^(j k)) * W[j p s],        W[k] = exp(-2 pi i k / n) from the table (conjugated for the inverse),
// j = 0 .. r - 1; j = 0 is not multiplied.  The r-point sums: radix 2 and 4 are adds and exact multiplications by +-i,
//     radix 4:  t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = a1 - a3;  b0 = t0 + t2, b2 = t0 - t2, b1 = t1 -+ i t3, b3 = t1 +- i t3;
// radices 3, 5 and 7 share one small-prime sum  b_j = ((a_0 + a_1 w^(j)) + a_2 w^(2j)) + ...  in ascending k with w^(jk) = W[((j k) % r) * (n / r)],
// b_0 = ((a_0 + a_1) + a_2) + ... without multiplications.  A complex product is (ar br - ai bi, ar bi + ai br), unfused.  x and y are two buffers:
// the result of pass i is the input of pass i + 1, so the result lies in the first buffer after an even number of passes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDBEDA_FFT_HD __host__ __device__
#else
#define PDBEDA_FFT_HD
#endif
#include <math.h>

#define PDBEDA_FFT_MAX_AXIS 1024
#define PDBEDA_FFT_MAX_PASSES 6

namespace pdbeda {

struct alignas(16) FftCplx { double re, im; };

struct FftPlan {
    int32_t n;
    int32_t n_pass;
    int32_t radix[PDBEDA_FFT_MAX_PASSES];
};

// The radix sequence of n (see above); false: n is not plannable (*plan is then untouched).
inline bool pdbeda_fft_plan(int64_t n, FftPlan *plan) {
    if (n < 1 || n > PDBEDA_FFT_MAX_AXIS) return false;
    FftPlan p;
    p.n = (int32_t)n;
    p.n_pass = 0;
    for (int k = 0; k < PDBEDA_FFT_MAX_PASSES; ++k) p.radix[k] = 1;
    int64_t rest = n;
    static const int order[5] = {4, 2, 3, 5, 7};
    for (int k = 0; k < 5; ++k)
        while (rest % order[k] == 0) {
            if (p.n_pass == PDBEDA_FFT_MAX_PASSES) return false;      // (cannot happen up to 1024)
            p.radix[p.n_pass++] = order[k];
            rest /= order[k];
        }
    if (rest != 1) return false;
    if (plan) *plan = p;
    return true;
}
inline bool pdbeda_fft_plannable(int64_t n) { return pdbeda_fft_plan(n, nullptr); }
// The next plannable length at or above n; 0 when there is none up to PDBEDA_FFT_MAX_AXIS.
inline int32_t pdbeda_fft_next(int64_t n) {
    for (int64_t k = n < 1 ? 1 : n; k <= PDBEDA_FFT_MAX_AXIS; ++k)
        if (pdbeda_fft_plannable(k)) return (int32_t)k;
    return 0;
}

// (host code.)  w[k] = exp(-2 pi i k / n), k = 0 .. n - 1, every component within 1 ulp.  The angle is reduced by whole quarter turns in integers, 4 k = q n + r with
// |r| <= n / 2, the remainder's sine and cosine (|angle| <= pi / 4) are taken in long double and rounded once, and the quarter turns are swaps and signs:
// w[0], w[n/4], w[n/2], w[3n/4] are exact, and the table has the symmetries of the circle down to its octants.
inline void pdbeda_fft_twiddles(int32_t n, FftCplx *w) {
    const long double half_pi = 1.57079632679489661923132169163975144L;
    for (int32_t k = 0; k < n; ++k) {
        const int64_t q = (8 * (int64_t)k + n) / (2 * (int64_t)n);
        const int64_t r = 4 * (int64_t)k - q * n;
        const long double phi = half_pi * (long double)r / (long double)n;
        const double c = r == 0 ? 1.0 : (double)cosl(phi), s = r == 0 ? 0.0 : (double)sinl(phi);
        double co, si;      // of the whole angle
        switch ((int)(q & 3)) {
            case 0: co = c; si = s; break;
            case 1: co = -s; si = c; break;
            case 2: co = -c; si = -s; break;
            default: co = s; si = -c; break;
        }
        w[k].re = co + 0.0;      // (+ 0.0: no negative zero in the table)
        w[k].im = -si + 0.0;
    }
}

PDBEDA_FFT_HD inline FftCplx fft_add(FftCplx a, FftCplx b) { return FftCplx{a.re + b.re, a.im + b.im}; }
PDBEDA_FFT_HD inline FftCplx fft_sub(FftCplx a, FftCplx b) { return FftCplx{a.re - b.re, a.im - b.im}; }
PDBEDA_FFT_HD inline FftCplx fft_mul(FftCplx a, FftCplx b) {
    const double rr = a.re * b.re, ii = a.im * b.im, ri = a.re * b.im, ir = a.im * b.re;
    return FftCplx{rr - ii, ri + ir};
}
// W[k] forward, its conjugate for the inverse.
PDBEDA_FFT_HD inline FftCplx fft_w(const FftCplx *w, int k, int inverse) {
    const FftCplx v = w[k];
    return inverse ? FftCplx{v.re, -v.im} : v;
}
// -i a (forward) or +i a (inverse).
PDBEDA_FFT_HD inline FftCplx fft_quarter(FftCplx a, int inverse) { return inverse ? FftCplx{-a.im, a.re} : FftCplx{a.im, -a.re}; }

// The r-point sum of a small prime r and the pass's twiddles (see the head of the file): one definition for 3, 5 and 7.
template <int R>
PDBEDA_FFT_HD inline void fft_prime(const FftCplx *in, FftCplx *out, int64_t in_step, int64_t out_step, int n, int ps, const FftCplx *w, int inverse) {
    FftCplx a[R];
    for (int k = 0; k < R; ++k) a[k] = in[k * in_step];
    const int root = n / R;
    FftCplx b = a[0];
    for (int k = 1; k < R; ++k) b = fft_add(b, a[k]);
    out[0] = b;
    for (int j = 1; j < R; ++j) {
        b = a[0];
        for (int k = 1; k < R; ++k) b = fft_add(b, fft_mul(a[k], fft_w(w, ((j * k) % R) * root, inverse)));
        out[j * out_step] = fft_mul(b, fft_w(w, j * ps, inverse));
    }
}

// Butterfly t (0 .. n / r - 1) of one pass on ONE line: x -> y, elements `es` apart (1 on the host; the lines of a tile are interleaved on the device).
// s: the product of the radices of the earlier passes; w: the table of the line's length n.
PDBEDA_FFT_HD inline void pdbeda_fft_butterfly(const FftCplx *x, FftCplx *y, int es, int n, int s, int r, int t, const FftCplx *w, int inverse) {
    const int m = n / (s * r);
    const int p = t / s, q = t - p * s;
    const FftCplx *in = x + (int64_t)(q + s * p) * es;
    FftCplx *out = y + (int64_t)(q + s * r * p) * es;
    const int64_t in_step = (int64_t)s * m * es, out_step = (int64_t)s * es;
    const int ps = p * s;      // W[j p s], j p s < n
    if (r == 4) {
        const FftCplx a0 = in[0], a1 = in[in_step], a2 = in[2 * in_step], a3 = in[3 * in_step];
        const FftCplx t0 = fft_add(a0, a2), t1 = fft_sub(a0, a2), t2 = fft_add(a1, a3), t3 = fft_quarter(fft_sub(a1, a3), inverse);
        out[0] = fft_add(t0, t2);
        out[out_step] = fft_mul(fft_add(t1, t3), fft_w(w, ps, inverse));
        out[2 * out_step] = fft_mul(fft_sub(t0, t2), fft_w(w, 2 * ps, inverse));
        out[3 * out_step] = fft_mul(fft_sub(t1, t3), fft_w(w, 3 * ps, inverse));
    } else if (r == 2) {
        const FftCplx a0 = in[0], a1 = in[in_step];
        out[0] = fft_add(a0, a1);
        out[out_step] = fft_mul(fft_sub(a0, a1), fft_w(w, ps, inverse));
    } else if (r == 3) {
        fft_prime<3>(in, out, in_step, out_step, n, ps, w, inverse);
    } else if (r == 5) {
        fft_prime<5>(in, out, in_step, out_step, n, ps, w, inverse);
    } else {
        fft_prime<7>(in, out, in_step, out_step, n, ps, w, inverse);
    }
}

// One whole line on the host (or by one device thread): x[n] -> the returned buffer, x or y, both of n elements and both overwritten.  Unnormalised.
PDBEDA_FFT_HD inline FftCplx *pdbeda_fft_line(FftCplx *x, FftCplx *y, const FftPlan &plan, const FftCplx *w, int inverse) {
    int s = 1;
    for (int i = 0; i < plan.n_pass; ++i) {
        const int r = plan.radix[i], nb = plan.n / r;
        for (int t = 0; t < nb; ++t) pdbeda_fft_butterfly(x, y, 1, plan.n, s, r, t, w, inverse);
        FftCplx *z = x; x = y; y = z;
        s *= r;
    }
    return x;
}

}  // namespace pdbeda
