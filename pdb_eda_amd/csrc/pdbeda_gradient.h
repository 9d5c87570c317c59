// pdbeda_gradient.h -- the way back from a map to the atoms: per atom and Gaussian term the sums of a weight map against the Gaussian, the Gaussian
// times the offset vector and the Gaussian times the squared distance (the adjoint of k_model_tile; the derivatives of a least-squares map-model
// target with respect to occupancy, position and B).  No reference counterpart; the contract is spelled out at pdbeda_atom_moments in
// include/pdbeda.h, the host's plan (checks, covering box, quantum) in pdbeda_gradplan.h.  Included from pdbeda_hip.hip.
//
//   k_atom_moments<NT>       ATOM-owned: a wave per atom, GP_WAVES atoms to a workgroup of 256, grid-strided over the atoms.  The lanes take the
//                            atom's clipped box (GradBox, from the host) GP_COLS x GP_ROWS = 16 x 4 voxels at a time, c fastest: a lane's column
//                            and row inside the trip are lane & 15 and lane >> 4, the trips walk c, then r, then s in wave-uniform loops, so no
//                            voxel costs a division and a row of the trip is one 64-byte read of the weight map.  The cheap reject d2 <= r2_hi
//                            comes before the root (the proof: pdbeda_model.h).  A lane keeps 5 * NT long long accumulators in registers (NT is
//                            a template parameter for that: indexed by a run-time term count they would live in scratch) and a pair count;
//                            every term is rounded once to 2^-S (fix_of).  The wave is folded AS INTEGERS by wave_fold<SegAdd>; lane i then
//                            writes output i with a plain vector store.  No atomic, no LDS, no floating-point sum across lanes or trips: the
//                            result of an atom depends on nothing but the atom, the map and S.
#pragma once
#include "pdbeda_gradplan.h"
#include "pdbeda_kernels.h"
#include "pdbeda_wave.h"

namespace pdbeda {

struct GradArgs {
    const Geom *geom;                    // of the weight map
    const float *w;                      // [ns][nr][nc]
    const double *xyz;                   // [n_atoms][3]
    const double *expo;                  // [n_atoms][NT]
    const float *radii;                  // [n_atoms]
    const GradBox *box;                  // [n_atoms], inside the stored box (the host clips)
    int n_atoms;
    double fix_mul, fix_inv;             // 2^S, 2^-S
    double *moments;                     // [n_atoms][NT][5]
    int32_t *n_voxels;                   // [n_atoms]
};

template <int NT>
__global__ void __launch_bounds__(256) k_atom_moments(GradArgs a) {
    const int lane = threadIdx.x & 63;
    const int col = lane & (GP_COLS - 1), row = lane >> 4;
    const Geom &g = *a.geom;
    const int64_t nc = g.ncrs[0], nr = g.ncrs[1];
    for (int64_t at = (int64_t)blockIdx.x * GP_WAVES + (threadIdx.x >> 6); at < a.n_atoms; at += (int64_t)gridDim.x * GP_WAVES) {      // (wave-uniform)
        const GradBox b = a.box[at];
        const double x = a.xyz[3 * at], y = a.xyz[3 * at + 1], z = a.xyz[3 * at + 2];
        const double rad = (double)a.radii[at];
        const double r2_hi = (rad * rad) * (1.0 + 0x1p-50);
        double k[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) k[j] = a.expo[at * NT + j];
        long long acc[NT][5];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[j][q] = 0;
        int count = 0;
        for (int ds = 0; ds < b.n[2]; ++ds)
            for (int r0 = 0; r0 < b.n[1]; r0 += GP_ROWS)
                for (int c0 = 0; c0 < b.n[0]; c0 += GP_COLS) {
                    const int dc = c0 + col, dr = r0 + row;
                    if (dc >= b.n[0] || dr >= b.n[1]) continue;
                    const int c = b.lo[0] + dc, r = b.lo[1] + dr, s = b.lo[2] + ds;
                    double p[3];
                    crs2xyz(g, c, r, s, p);
                    const double dx = p[0] - x, dy = p[1] - y, dz = p[2] - z;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 <= r2_hi)) continue;
                    if (!(__dsqrt_rn(d2) <= rad)) continue;
                    const double w = (double)a.w[((int64_t)s * nr + r) * nc + c];
                    ++count;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const double e = k[j] * d2;
                        const double t0 = w * exp(-e);
                        acc[j][0] += fix_of(t0, a.fix_mul);
                        acc[j][1] += fix_of(t0 * dx, a.fix_mul);
                        acc[j][2] += fix_of(t0 * dy, a.fix_mul);
                        acc[j][3] += fix_of(t0 * dz, a.fix_mul);
                        acc[j][4] += fix_of(t0 * d2, a.fix_mul);
                    }
                }
        count = wave_fold<SegAdd>(count);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const long long sum = wave_fold<SegAdd>(acc[j][q]);
                if (lane == 5 * j + q) a.moments[(at * NT + j) * 5 + q] = (double)sum * a.fix_inv;      // (a power of two: exact; 0 -> +0.0)
            }
        if (lane == 63) a.n_voxels[at] = count;
    }
}

}  // namespace pdbeda
