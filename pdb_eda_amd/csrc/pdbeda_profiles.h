// pdbeda_profiles.h -- radial density profiles: per atom, the voxels and the density of n_shells concentric shells out to one radius.
// No reference counterpart (the reference answers "what is inside ONE radius"); the contract is spelled out at pdbeda_radial_profiles
// in include/pdbeda.h.
//
//   k_atom_shells    a workgroup per atom, grid-strided: ONE pass over the atom's sphere box [C-R-1, C+R] with the voxel -> thread
//                    mapping, the sphere test, the wrapped fetch and the validity flag of k_atom_region; a voxel inside the sphere
//                    goes to shell min(floor(d / w), n_shells - 1), w = radius / n_shells (IEEE divisions: membership is compared
//                    bit for bit).
//
// The shell tables live in LDS and are folded with INTEGER atomics: a voxel's density is rounded once to the map's fixed-point
// quantum (fix_of, the FixSums idea of pdbeda_kernels.h) and integer addition commutes, so the sums do not depend on the order
// the hardware serves the atomics in -- bit-identical from run to run.  Every wave has tables of its own (neighbouring lanes
// along c mostly hit the same shell, and four waves on one table would queue behind each other as well); they are merged after
// a barrier by one thread per shell, which writes the [n_atoms][n_shells] rows with plain vector stores.
// Priced and dropped: summing the lanes that hold consecutive voxels of the same shell across lanes first, so
// that only the first lane of each such run issues the atomics -- a row of a sphere box is a dozen voxels and crosses several
// shells, so the runs are one to three lanes long and the six shuffle steps cost more than the atomics they save.
#pragma once
#include "pdbeda_kernels.h"

namespace pdbeda {

static constexpr int SHELL_WAVES = 4;      // waves of a workgroup of 256

__global__ void __launch_bounds__(256) k_atom_shells(const Geom *__restrict__ gp, const float *__restrict__ dens, const double *__restrict__ xyz,
                                                     const AtomBox *__restrict__ boxes, int n_atoms, float radius, int n_shells, float cutoff,
                                                     double fix_mul, double fix_inv, long long *__restrict__ out_n, double *__restrict__ out_sum,
                                                     long long *__restrict__ out_nsig, double *__restrict__ out_sumsig, uint8_t *__restrict__ out_valid) {
    __shared__ unsigned long long s_sum[SHELL_WAVES][PDBEDA_MAX_SHELLS], s_sumsig[SHELL_WAVES][PDBEDA_MAX_SHELLS];
    __shared__ unsigned int s_n[SHELL_WAVES][PDBEDA_MAX_SHELLS], s_nsig[SHELL_WAVES][PDBEDA_MAX_SHELLS];
    __shared__ unsigned int s_bad[SHELL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Geom &g = *gp;
    const double rad = (double)radius, cut = (double)cutoff;
    const double w = __ddiv_rn(rad, (double)n_shells);
    const bool all_sig = !(cut > 0.0) && !(cut < 0.0);      // cutoff 0: every voxel passes -- the significant columns ARE the plain ones
    if (tid < PDBEDA_MAX_SHELLS)
        for (int k = 0; k < SHELL_WAVES; ++k) { s_sum[k][tid] = 0ull; s_sumsig[k][tid] = 0ull; s_n[k][tid] = 0u; s_nsig[k][tid] = 0u; }
    __syncthreads();
    for (int v = blockIdx.x; v < n_atoms; v += gridDim.x) {
        const AtomBox bx = boxes[v];
        const double px = xyz[3 * v], py = xyz[3 * v + 1], pz = xyz[3 * v + 2];
        // (an empty box is lo 0 / hi -1 along every axis: no voxel.  The host has refused a box of 2^31 voxels or more)
        const unsigned dc = (unsigned)(bx.hi[0] - bx.lo[0] + 1), dr = (unsigned)(bx.hi[1] - bx.lo[1] + 1);
        const unsigned nvox = dc * dr * (unsigned)(bx.hi[2] - bx.lo[2] + 1);
        bool bad = false;
        for (unsigned base = 0; base < nvox; base += 256u) {
            const unsigned i = base + (unsigned)tid;
            int shell = -1;
            long long F = 0;
            bool sig = false;
            if (i < nvox) {
                const unsigned row = i / dc, c = i - row * dc, sl = row / dr, rl = row - sl * dr;
                const int rc = bx.lo[0] + (int)c, rr = bx.lo[1] + (int)rl, rs = bx.lo[2] + (int)sl;
                double p[3];
                crs2xyz(g, rc, rr, rs, p);
                const double dx = p[0] - px, dy = p[1] - py, dz = p[2] - pz;
                const double d = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
                if (d <= rad) {
                    bool ok = true;
                    const double rho = (double)fetch_wrapped(g, dens, rc, rr, rs, &ok);
                    bad = bad || !ok;
                    shell = min((int)floor(__ddiv_rn(d, w)), n_shells - 1);
                    F = fix_of(rho, fix_mul);
                    sig = all_sig || (cut > 0.0 ? rho > cut : rho < cut);
                }
            }
            if (shell >= 0) {
                atomicAdd(&s_n[wv][shell], 1u);
                atomicAdd(&s_sum[wv][shell], (unsigned long long)F);
                if (!all_sig && sig) {
                    atomicAdd(&s_nsig[wv][shell], 1u);
                    atomicAdd(&s_sumsig[wv][shell], (unsigned long long)F);
                }
            }
        }
        const unsigned long long any_bad = __ballot(bad);
        if (lane == 0) s_bad[wv] = any_bad ? 1u : 0u;
        __syncthreads();
        if (tid < n_shells) {      // one thread per shell: the waves' tables merged (integers: any order), written, and cleared for the next atom
            unsigned int n = 0, ns = 0;
            long long S = 0, T = 0;
            for (int k = 0; k < SHELL_WAVES; ++k) {
                n += s_n[k][tid]; ns += s_nsig[k][tid]; S += (long long)s_sum[k][tid]; T += (long long)s_sumsig[k][tid];
                s_n[k][tid] = 0u; s_nsig[k][tid] = 0u; s_sum[k][tid] = 0ull; s_sumsig[k][tid] = 0ull;
            }
            if (all_sig) { ns = n; T = S; }
            const size_t o = (size_t)v * (size_t)n_shells + (size_t)tid;
            out_n[o] = (long long)n;
            out_sum[o] = (double)S * fix_inv;      // (a power of two: the product is exact)
            out_nsig[o] = (long long)ns;
            out_sumsig[o] = (double)T * fix_inv;
        }
        if (tid == 0) out_valid[v] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 0 : 1;
        __syncthreads();
    }
}

}  // namespace pdbeda
