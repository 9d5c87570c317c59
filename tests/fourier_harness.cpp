// fourier_harness.cpp -- pdb_eda_amd/csrc/pdbeda_fourier_line.h on a CPU: a stand-alone program for the host compiler and its sanitizers
// (tests/test_fourier_host.py) that runs the planner, the twiddle table and the line transform the device runs, and restates the 3-D forward
// transform of pdbeda_map_fft in the device's order (tests/test_gpu_fourier.py compares the device's spectrum with it TO THE BIT).
//
//   fourier_harness plan  LO HI            one text line per n in LO .. HI: "n plannable next n_pass radices..."
//   fourier_harness lines IN OUT           IN: int32 count, then per line int32 n and n complex128.  OUT: per line n complex128 forward, n complex128
//                                          inverse (unnormalised), n complex128 twiddle table.  A length that is not plannable ends the run with status 3.
//   fourier_harness volume IN OUT          IN: int32 nc, nr, ns, then [ns][nr][nc] float32.  OUT: [ns][nr][nc / 2 + 1] complex128, the half spectrum.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pdbeda_fourier_line.h"

using namespace pdbeda;

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static bool write_all(FILE *f, const void *src, size_t bytes) { return bytes == 0 || fwrite(src, 1, bytes, f) == bytes; }

static int run_plan(long lo, long hi) {
    for (long n = lo; n <= hi; ++n) {
        FftPlan p;
        const bool ok = pdbeda_fft_plan(n, &p);
        printf("%ld %d %d", n, ok ? 1 : 0, (int)pdbeda_fft_next(n));
        if (ok) {
            printf(" %d", p.n_pass);
            long prod = 1;
            for (int k = 0; k < p.n_pass; ++k) { printf(" %d", p.radix[k]); prod *= p.radix[k]; }
            if (prod != n || p.n != n) return 4;
        }
        printf("\n");
    }
    return 0;
}

static int run_lines(const char *in_path, const char *out_path) {
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    int32_t count = 0;
    if (!read_all(in, &count, 4)) return 2;
    for (int32_t c = 0; c < count; ++c) {
        int32_t n = 0;
        if (!read_all(in, &n, 4)) return 2;
        FftPlan plan;
        if (!pdbeda_fft_plan(n, &plan)) return 3;
        std::vector<FftCplx> line((size_t)n), x((size_t)n), y((size_t)n), w((size_t)n);
        if (!read_all(in, line.data(), sizeof(FftCplx) * (size_t)n)) return 2;
        pdbeda_fft_twiddles(n, w.data());
        for (int inverse = 0; inverse < 2; ++inverse) {
            x = line;
            const FftCplx *res = pdbeda_fft_line(x.data(), y.data(), plan, w.data(), inverse);
            if (!write_all(out, res, sizeof(FftCplx) * (size_t)n)) return 2;
        }
        if (!write_all(out, w.data(), sizeof(FftCplx) * (size_t)n)) return 2;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

// One strided line of a [ns][nr][nh] volume, in place through two line buffers.
static void line_in_place(FftCplx *vol, int64_t first, int64_t stride, const FftPlan &plan, const FftCplx *w, std::vector<FftCplx> &x, std::vector<FftCplx> &y) {
    for (int i = 0; i < plan.n; ++i) x[(size_t)i] = vol[first + i * stride];
    const FftCplx *res = pdbeda_fft_line(x.data(), y.data(), plan, w, 0);
    for (int i = 0; i < plan.n; ++i) vol[first + i * stride] = res[i];
}

static int run_volume(const char *in_path, const char *out_path) {
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    if (!in || !out) return 2;
    int32_t ncrs[3];
    if (!read_all(in, ncrs, 12)) return 2;
    FftPlan plan[3];
    std::vector<FftCplx> w[3];
    int longest = 1;
    for (int k = 0; k < 3; ++k) {
        if (!pdbeda_fft_plan(ncrs[k], &plan[k])) return 3;
        w[k].resize((size_t)ncrs[k]);
        pdbeda_fft_twiddles(ncrs[k], w[k].data());
        if (ncrs[k] > longest) longest = ncrs[k];
    }
    const int nc = ncrs[0], nr = ncrs[1], ns = ncrs[2], nh = nc / 2 + 1;
    std::vector<float> map((size_t)nc * nr * ns);
    if (!read_all(in, map.data(), 4 * map.size())) return 2;
    std::vector<FftCplx> vol((size_t)nh * nr * ns), x((size_t)longest), y((size_t)longest);
    for (int64_t row = 0; row < (int64_t)nr * ns; ++row) {      // along c: the row as a complex line with zero imaginary parts, columns 0 .. nc / 2 kept
        for (int i = 0; i < nc; ++i) x[(size_t)i] = FftCplx{(double)map[(size_t)(row * nc + i)], 0.0};
        const FftCplx *res = pdbeda_fft_line(x.data(), y.data(), plan[0], w[0].data(), 0);
        for (int h = 0; h < nh; ++h) vol[(size_t)(row * nh + h)] = res[h];
    }
    for (int s = 0; s < ns; ++s)      // along r
        for (int h = 0; h < nh; ++h) line_in_place(vol.data(), (int64_t)s * nr * nh + h, nh, plan[1], w[1].data(), x, y);
    for (int r = 0; r < nr; ++r)      // along s
        for (int h = 0; h < nh; ++h) line_in_place(vol.data(), (int64_t)r * nh + h, (int64_t)nh * nr, plan[2], w[2].data(), x, y);
    if (!write_all(out, vol.data(), sizeof(FftCplx) * vol.size())) return 2;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "plan") == 0) return run_plan(atol(argv[2]), atol(argv[3]));
    if (argc == 4 && strcmp(argv[1], "lines") == 0) return run_lines(argv[2], argv[3]);
    if (argc == 4 && strcmp(argv[1], "volume") == 0) return run_volume(argv[2], argv[3]);
    fprintf(stderr, "usage: fourier_harness plan LO HI | lines IN OUT | volume IN OUT\n");
    return 1;
}
