// Crystal contacts (crystalContacts.py of the reference) without pymol: the counting sort of a point set into a uniform cell grid (pdbeda_cellgrid.h:
// count, scan, scatter -- the sort of every atom-grid entry point), the symmetry images of the asymmetric unit's polymer atoms that come within the
// cutoff of it, and the minimum distance of every query point to the atoms of the kept images.  Included from pdbeda_hip.hip.  All coordinates and
// distances are fp64; a distance is scipy cdist's sqrt((dx*dx + dy*dy) + dz*dz) (the library builds with -ffp-contract=off), as k_nearest_atom computes it.
#pragma once
#include "pdbeda_kernels.h"
#include "pdbeda_cellgrid.h"

namespace pdbeda {

__device__ inline double contact_dist(const double a[3], const double *__restrict__ b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
}

// Image g = (op, n) of p: R_op p + t_op + orthoMat n, with symmetry_candidate's arithmetic (the same coordinates for |n| <= 1).
// cand = (op, n0, n1, n2).
__device__ inline void image_point(const double *__restrict__ rot, const double *__restrict__ ortho, const int32_t *__restrict__ cand, const double p[3], double v[3]) {
    const double n[3] = {(double)cand[1], (double)cand[2], (double)cand[3]};
    double ot[3];
    matvec3(ortho, n, ot);
    const double *rm = rot + 12 * cand[0];
    for (int q = 0; q < 3; ++q) {
        double w = ((rm[4 * q] * p[0] + rm[4 * q + 1] * p[1]) + rm[4 * q + 2] * p[2]);
        w = (w + rm[4 * q + 3]) + ot[q];
        v[q] = w;
    }
}

// ---- counting sort of a point list into a grid: count, scan, scatter ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_grid_count_points(const double *__restrict__ xyz, int64_t n, CellGrid g, unsigned *__restrict__ count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (grid_cropped(g, v)) continue;
        atomicAdd(&count[grid_cell(g, v)], 1u);
    }
}

// Within a cell the order of the points depends on the atomics; a minimum distance does not.  `room` bounds every write.  INDEXED: each point's
// ORIGINAL index goes with it (a tie rule by atom index needs it, and so do per-atom rows).  Two kernel names over one body: profiles key on them.
template <bool INDEXED>
__device__ inline void grid_scatter(const double *__restrict__ xyz, int64_t n, const CellGrid &g, unsigned *__restrict__ cursor, double *__restrict__ sorted, int *__restrict__ sorted_index, int64_t room) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (grid_cropped(g, v)) continue;
        const unsigned pos = atomicAdd(&cursor[grid_cell(g, v)], 1u);
        if ((int64_t)pos < room) { sorted[3 * pos] = v[0]; sorted[3 * pos + 1] = v[1]; sorted[3 * pos + 2] = v[2]; if (INDEXED) sorted_index[pos] = (int)i; }
    }
}
__global__ void __launch_bounds__(256) k_grid_scatter_points(const double *__restrict__ xyz, int64_t n, CellGrid g, unsigned *__restrict__ cursor, double *__restrict__ sorted, int64_t room) {
    grid_scatter<false>(xyz, n, g, cursor, sorted, nullptr, room);
}
__global__ void __launch_bounds__(256) k_grid_scatter_indexed(const double *__restrict__ xyz, int64_t n, CellGrid g, unsigned *__restrict__ cursor, double *__restrict__ sorted,
                                                              int *__restrict__ sorted_index, int64_t room) {
    grid_scatter<true>(xyz, n, g, cursor, sorted, sorted_index, room);
}

// Inclusive scan of one value per lane across a 1024-lane block; `total` gets the block's sum.
// (its wave scan is wave_incl_scan's loop, kept here: on the shared one k_contact_compact measured 0.4 % slower)
__device__ inline unsigned block_scan_1024(unsigned x, unsigned *s_wave, unsigned &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
        const unsigned t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();      // (s_wave is written again by the next call)
    total = all;
    return before + x;
}

// Exclusive scan of the cell counts in ONE block (8 cells per lane per tile): start[c] = cursor[c] = points before cell c, start[n] = all
// (also into *total_out when given: the pinned block).
__global__ void __launch_bounds__(1024) k_grid_scan(const unsigned *__restrict__ count, int n, unsigned *__restrict__ start, unsigned *__restrict__ cursor,
                                                    unsigned *__restrict__ total_out) {
    __shared__ unsigned s_wave[16];
    unsigned carry = 0;
    for (int base = 0; base < n; base += 8 * 1024) {
        const int i0 = base + 8 * (int)threadIdx.x;
        unsigned v[8], sum = 0;
        for (int k = 0; k < 8; ++k) { v[k] = i0 + k < n ? count[i0 + k] : 0u; sum += v[k]; }
        unsigned tile = 0;
        unsigned run = carry + block_scan_1024(sum, s_wave, tile) - sum;
        for (int k = 0; k < 8; ++k)
            if (i0 + k < n) { start[i0 + k] = run; cursor[i0 + k] = run; run += v[k]; }
        carry += tile;
    }
    if (threadIdx.x == 0) {
        start[n] = carry;
        if (total_out) *total_out = carry;
    }
}

// ---- images ---------------------------------------------------------------------------------------------------------------------------------
// One lane per (candidate image c, polymer atom j): image c is kept (keep[c] = 1) when g_c(x_j) lies within the cutoff of a polymer atom of the
// asymmetric unit (the grid over P).  The flag is only ever raised, so the result does not depend on lane order; a lane whose image is kept
// already stops at once.
__global__ void __launch_bounds__(256) k_image_select(const double *__restrict__ poly, int64_t n_poly, const double *__restrict__ rot, const double *__restrict__ ortho,
                                                      const int32_t *__restrict__ cand, int64_t n_cand, const double *__restrict__ sorted, const unsigned *__restrict__ start,
                                                      CellGrid g, double cutoff, unsigned *keep) {
    const int64_t total = n_cand * n_poly;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = t / n_poly, j = t - c * n_poly;
        if (*(volatile unsigned *)&keep[c]) continue;
        const double p[3] = {poly[3 * j], poly[3 * j + 1], poly[3 * j + 2]};
        double v[3];
        image_point(rot, ortho, cand + 4 * c, p, v);
        int lo[3], hi[3];
        if (!grid_range(g, v, lo, hi)) continue;
        bool hit = false;
        for_each_cell_row(g, start, lo, hi, [&](unsigned b, unsigned e) {
            for (unsigned k = b; k < e; ++k)
                if (contact_dist(v, sorted + 3 * k) <= cutoff) { hit = true; break; }
            return hit;
        });
        if (hit) keep[c] = 1u;
    }
}

// The kept images' atoms counted into / scattered over the grid over the neighbour set (lanes (c, j) again, the same arithmetic).  The count
// also hands the keep flags to the host (keep_out, the pinned block, when given).
__global__ void __launch_bounds__(256) k_image_count(const double *__restrict__ poly, int64_t n_poly, const double *__restrict__ rot, const double *__restrict__ ortho,
                                                     const int32_t *__restrict__ cand, int64_t n_cand, const unsigned *__restrict__ keep, CellGrid g, unsigned *__restrict__ count,
                                                     unsigned *__restrict__ keep_out) {
    const int64_t total = n_cand * n_poly;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = t / n_poly, j = t - c * n_poly;
        if (j == 0 && keep_out) keep_out[c] = keep[c];
        if (!keep[c]) continue;
        const double p[3] = {poly[3 * j], poly[3 * j + 1], poly[3 * j + 2]};
        double v[3];
        image_point(rot, ortho, cand + 4 * c, p, v);
        if (grid_cropped(g, v)) continue;
        atomicAdd(&count[grid_cell(g, v)], 1u);
    }
}

__global__ void __launch_bounds__(256) k_image_scatter(const double *__restrict__ poly, int64_t n_poly, const double *__restrict__ rot, const double *__restrict__ ortho,
                                                       const int32_t *__restrict__ cand, int64_t n_cand, const unsigned *__restrict__ keep, CellGrid g,
                                                       unsigned *__restrict__ cursor, double *__restrict__ sorted, int64_t room) {
    const int64_t total = n_cand * n_poly;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = t / n_poly, j = t - c * n_poly;
        if (!keep[c]) continue;
        const double p[3] = {poly[3 * j], poly[3 * j + 1], poly[3 * j + 2]};
        double v[3];
        image_point(rot, ortho, cand + 4 * c, p, v);
        if (grid_cropped(g, v)) continue;
        const unsigned pos = atomicAdd(&cursor[grid_cell(g, v)], 1u);
        if ((int64_t)pos < room) { sorted[3 * pos] = v[0]; sorted[3 * pos + 1] = v[1]; sorted[3 * pos + 2] = v[2]; }
    }
}

// simulateCrystalNeighborCoordinates' list: the atoms of the listed images in (image, atom) order.
__global__ void __launch_bounds__(256) k_image_emit(const double *__restrict__ poly, int64_t n_poly, const double *__restrict__ rot, const double *__restrict__ ortho,
                                                    const int32_t *__restrict__ cand, int64_t n_cand, double *__restrict__ out) {
    const int64_t total = n_cand * n_poly;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = t / n_poly, j = t - c * n_poly;
        const double p[3] = {poly[3 * j], poly[3 * j + 1], poly[3 * j + 2]};
        double v[3];
        image_point(rot, ortho, cand + 4 * c, p, v);
        out[3 * t] = v[0]; out[3 * t + 1] = v[1]; out[3 * t + 2] = v[2];
    }
}

// ---- contacts ---------------------------------------------------------------------------------------------------------------------------------
// Lane per query: the minimum distance to the gridded points of its 27 cells (INFINITY when there are none).  A point outside those cells is
// farther than the cutoff, so the minimum is exact whenever it is <= cutoff -- the only case that is reported.
__global__ void __launch_bounds__(256) k_contact_min(const double *__restrict__ q, int64_t n_q, const double *__restrict__ sorted, const unsigned *__restrict__ start,
                                                     CellGrid g, double *__restrict__ dist) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_q; i += (int64_t)gridDim.x * blockDim.x) {
        const double v[3] = {q[3 * i], q[3 * i + 1], q[3 * i + 2]};
        double best = INFINITY;
        int lo[3], hi[3];
        if (grid_range(g, v, lo, hi))
            for_each_cell_row(g, start, lo, hi, [&](unsigned b, unsigned e) {
                for (unsigned k = b; k < e; ++k) best = fmin(best, contact_dist(v, sorted + 3 * k));
                return false;
            });
        dist[i] = best;
    }
}

// The queries with dist <= cutoff as (index, distance) in ascending index order, in ONE block; at most `cap` rows are written, n_out gets
// how many there are.
__global__ void __launch_bounds__(1024) k_contact_compact(const double *__restrict__ dist, int64_t n_q, double cutoff, int64_t *__restrict__ out_index,
                                                          double *__restrict__ out_dist, int64_t cap, int64_t *__restrict__ n_out) {
    __shared__ unsigned s_wave[16];
    int64_t carry = 0;
    for (int64_t base = 0; base < n_q; base += 8 * 1024) {
        const int64_t i0 = base + 8 * (int64_t)threadIdx.x;
        unsigned hits = 0;
        for (int k = 0; k < 8; ++k) hits += (i0 + k < n_q && dist[i0 + k] <= cutoff) ? 1u : 0u;
        unsigned tile = 0;
        int64_t pos = carry + (int64_t)(block_scan_1024(hits, s_wave, tile) - hits);
        for (int k = 0; k < 8; ++k)
            if (i0 + k < n_q && dist[i0 + k] <= cutoff) {
                if (pos < cap) { out_index[pos] = i0 + k; out_dist[pos] = dist[i0 + k]; }
                ++pos;
            }
        carry += tile;
    }
    if (threadIdx.x == 0) *n_out = carry;
}

}  // namespace pdbeda
