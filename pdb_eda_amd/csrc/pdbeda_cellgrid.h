// pdbeda_cellgrid.h -- the uniform cell grid every atom-grid entry point sorts its points into (pdbeda_coord_contacts, pdbeda_crystal_contacts,
// pdbeda_map_partition, pdbeda_atom_qscores, pdbeda_model_density): the grid and its cell rule, the host's planner of a grid, and the device's walks
// over the cells near a query.  Host and device code: hipcc compiles it into the kernels (pdbeda_contacts.h), a plain C++17 compiler into the host
// library's planning and into tests/cellgrid_harness.cpp, which runs the planner on a CPU under sanitizers.  DESIGN.md 4.13.
#pragma once
#include "pdbeda_device.h"

#include <algorithm>
#include <cmath>

namespace pdbeda {

// A uniform grid: cell (cx, cy, cz) = floor((x - lo) / edge) per axis, cell number (cz * dim[1] + cy) * dim[0] + cx.  edge > cutoff
// (strictly, with a relative margin far above the rounding of the division): two points within the cutoff of each other lie in the same
// or in adjacent cells, so the 27 cells around a point hold every point within the cutoff of it.  Points that lie outside the crop box
// are not gridded (the box is the query set's bounding box grown by more than the cutoff: no such point can be within the cutoff of a
// query); points inside it whose cell falls outside [0, dim) by rounding are clamped to the border cell, which keeps adjacent cells adjacent.
struct CellGrid {
    double lo[3];
    double edge;
    double crop_lo[3], crop_hi[3];
    int dim[3];
    int n_cells;
};

__host__ __device__ inline bool grid_cropped(const CellGrid &g, const double v[3]) {
    return !(v[0] >= g.crop_lo[0] && v[0] <= g.crop_hi[0] && v[1] >= g.crop_lo[1] && v[1] <= g.crop_hi[1] && v[2] >= g.crop_lo[2] && v[2] <= g.crop_hi[2]);
}

__host__ __device__ inline int grid_cell(const CellGrid &g, const double v[3]) {
    int c[3];
    for (int q = 0; q < 3; ++q) {
        const double f = floor((v[q] - g.lo[q]) / g.edge);
        c[q] = f < 0.0 ? 0 : (f > (double)(g.dim[q] - 1) ? g.dim[q] - 1 : (int)f);
    }
    return (c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0];
}

// The cells a point at v has to search: its own cell +- 1 per axis, inside the grid.  False when no gridded point can be within the cutoff.
__host__ __device__ inline bool grid_range(const CellGrid &g, const double v[3], int lo[3], int hi[3]) {
    for (int q = 0; q < 3; ++q) {
        const double f = floor((v[q] - g.lo[q]) / g.edge);
        if (!(f >= -1.0 && f <= (double)g.dim[q])) return false;
        const int c = (int)f;
        lo[q] = c - 1 < 0 ? 0 : c - 1;
        hi[q] = c + 1 > g.dim[q] - 1 ? g.dim[q] - 1 : c + 1;
    }
    return true;
}

// The xyz bounding box of the crs box [c0, c1] (inclusive): of its 8 corners -- crs2xyz is affine, so that is right on skewed cells too.
__host__ __device__ inline void crs_box_xyz(const Geom &g, const int32_t c0[3], const int32_t c1[3], double lo[3], double hi[3]) {
    for (int q = 0; q < 3; ++q) { lo[q] = INFINITY; hi[q] = -INFINITY; }
    for (int k = 0; k < 8; ++k) {
        double p[3];
        crs2xyz(g, (k & 1) ? c1[0] : c0[0], (k & 2) ? c1[1] : c0[1], (k & 4) ? c1[2] : c0[2], p);
        for (int q = 0; q < 3; ++q) { lo[q] = fmin(lo[q], p[q]); hi[q] = fmax(hi[q], p[q]); }
    }
}

// ---- the host's planner -------------------------------------------------------------------------------------------------------------------
// What it promises: a grid of at least one cell and at most 2^22, whose edge is above the cutoff, for every box of finite, non-negative extent
// -- and a refusal, not a loop without end, for any other.  It runs with -ffp-contract=off like the rest of the library: the device repeats the
// cell rule on what it makes.
inline void bbox3(const double *xyz, int64_t n, double lo[3], double hi[3]) {
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};      // (locals: in registers whatever lo and hi may alias)
    for (int64_t i = 0; i < n; ++i)
        for (int q = 0; q < 3; ++q) { l[q] = std::min(l[q], xyz[3 * i + q]); h[q] = std::max(h[q], xyz[3 * i + q]); }
    for (int q = 0; q < 3; ++q) { lo[q] = l[q]; hi[q] = h[q]; }
}

// The first axis along which hi - lo is negative (no point), NaN or infinite (finite ends whose difference overflows fp64, +-1e308); -1: none.
inline int bad_extent(const double lo[3], const double hi[3]) {
    for (int q = 0; q < 3; ++q)
        if (!(hi[q] - lo[q] >= 0.0 && std::isfinite(hi[q] - lo[q]))) return q;
    return -1;
}

// Grid over the box [lo, hi]: edge just above the cutoff, enlarged until the cells number at most 8 per point (at least 4096, at most 2^22: the
// single-block scan stays short, and a box that is huge beside the cutoff costs longer cell lists, never an overflowing dimension).  Correctness only
// needs edge > cutoff.  false: bad_extent -- with an infinite extent the cell count is inf, then NaN once the edge is, and the loop would never end.
inline bool make_cell_grid(const double lo[3], const double hi[3], double cutoff, int64_t n_points, const double crop_lo[3], const double crop_hi[3], CellGrid *out) {
    if (bad_extent(lo, hi) >= 0) return false;
    const double cap = (double)std::min<int64_t>(1 << 22, std::max<int64_t>(4096, 8 * n_points));
    double edge = cutoff * (1.0 + 1e-6);
    for (;;) {
        double cells = 1.0;
        for (int q = 0; q < 3; ++q) cells *= std::floor((hi[q] - lo[q]) / edge) + 1.0;
        if (cells <= cap) break;
        edge *= 1.25;
    }
    CellGrid g;
    g.edge = edge;
    g.n_cells = 1;
    for (int q = 0; q < 3; ++q) {
        g.lo[q] = lo[q];
        g.dim[q] = (int)std::floor((hi[q] - lo[q]) / edge) + 1;
        g.n_cells *= g.dim[q];
        g.crop_lo[q] = crop_lo[q];
        g.crop_hi[q] = crop_hi[q];
    }
    *out = g;
    return true;
}

// The grid a query set searches: over its bounding box grown by twice the cutoff ([lo, hi], handed back to name a refusal by), also the crop box of its points.
inline bool query_grid(const double *q_xyz, int64_t n_q, double cutoff, int64_t n_points, CellGrid *out, double lo[3], double hi[3]) {
    bbox3(q_xyz, n_q, lo, hi);
    for (int q = 0; q < 3; ++q) { lo[q] -= 2 * cutoff; hi[q] += 2 * cutoff; }
    return make_cell_grid(lo, hi, cutoff, n_points, lo, hi, out);
}

// The grid of the atoms that can matter to a box [blo, bhi] in xyz: the crop box is the box grown by the reach (and by a margin wider than a tile's
// own, tile_cell_range) -- an atom outside it reaches nothing in the box --, and the grid lies over its intersection with the atoms' bounding box, so it
// never grows with atoms that lie far from the box.  No atom, or an atoms' box beside the crop box: one cell, and no atom in it.  (The scored atoms of
// pdbeda_atom_qscores lie in both boxes: that call never meets the empty rule.)  The edge is just above the reach.  false: as make_cell_grid, which
// a finite [blo, bhi] and reach cannot cause.
inline bool crop_cell_grid(const double blo[3], const double bhi[3], double reach, const double *xyz, int64_t n_atoms, CellGrid *out) {
    double crop_lo[3], crop_hi[3], alo[3], ahi[3], glo[3], ghi[3];
    bbox3(xyz, n_atoms, alo, ahi);
    bool empty = n_atoms == 0;
    for (int q = 0; q < 3; ++q) {
        const double pad = reach * (1.0 + 1e-5) + 1e-8 * (std::fabs(blo[q]) + std::fabs(bhi[q]) + 1.0);
        crop_lo[q] = blo[q] - pad; crop_hi[q] = bhi[q] + pad;
        glo[q] = std::max(crop_lo[q], alo[q]); ghi[q] = std::min(crop_hi[q], ahi[q]);
        if (!(glo[q] <= ghi[q])) empty = true;
    }
    if (empty)
        for (int q = 0; q < 3; ++q) glo[q] = ghi[q] = crop_lo[q];
    return make_cell_grid(glo, ghi, reach, n_atoms, crop_lo, crop_hi, out);
}

// A reach spans fewer than 2^29 steps of every grid axis: what lies within it of a castable point stays castable (int32 indices, with room to add).
inline bool reach_below_2p29_steps(const Geom &g, double reach) {
    for (int i = 0; i < 3; ++i) {
        const double per_unit = g.orthogonal ? 1.0 / std::fabs(g.grid_len[i])
                                             : (std::fabs(g.deortho[3 * i]) + std::fabs(g.deortho[3 * i + 1]) + std::fabs(g.deortho[3 * i + 2])) * (double)g.xyz_interval[i];
        if (!(reach * per_unit < (double)(1ll << 29))) return false;
    }
    return true;
}

#if defined(__HIPCC__)
// ---- the device's walks (workgroups of 256) ---------------------------------------------------------------------------------------------
// Every row of cells of [lo, hi]: f(b, e) gets the sorted positions [b, e) of the row's points -- cells lo[0]..hi[0] of a row are consecutive in
// the counting sort -- and returns true to end the walk.
template <typename F>
__device__ inline void for_each_cell_row(const CellGrid &g, const unsigned *__restrict__ start, const int lo[3], const int hi[3], F f) {
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            const int row = (z * g.dim[1] + y) * g.dim[0];      // (a grid has at most 2^22 cells)
            if (f(start[row + lo[0]], start[row + hi[0] + 1])) return;
        }
}

// A tile of C x R x S voxels (powers of two, 256 in all) of a box of n[3] voxels, one thread per voxel (c fastest): tile number =
// (ts * tiles_r + tr) * tiles_c + tc.
struct TileVoxel { int32_t c0[3], c1[3]; int c, r, s; bool live; };      // the tile's corners, clamped to the box; the thread's voxel, and whether it lies in the box
template <int C, int R, int S>
__device__ inline TileVoxel tile_voxel(int64_t tile, int tiles_c, int tiles_r, const int n[3], int tid) {
    const int tc = (int)(tile % tiles_c), tr = (int)((tile / tiles_c) % tiles_r), ts = (int)(tile / ((int64_t)tiles_c * tiles_r));
    TileVoxel t;
    t.c0[0] = tc * C; t.c0[1] = tr * R; t.c0[2] = ts * S;
    t.c1[0] = min(t.c0[0] + C, n[0]) - 1; t.c1[1] = min(t.c0[1] + R, n[1]) - 1; t.c1[2] = min(t.c0[2] + S, n[2]) - 1;
    t.c = t.c0[0] + (tid & (C - 1)); t.r = t.c0[1] + ((tid / C) & (R - 1)); t.s = t.c0[2] + tid / (C * R);
    t.live = t.c < n[0] && t.r < n[1] && t.s < n[2];
    return t;
}

// The cells a tile has to search: its corners' bounding box, grown by the reach and by a margin far above the rounding of crs2xyz and of the
// distance (an interior voxel may leave the corners' box by an ulp; the cell of a point is monotonic in it).  false: beside the grid, or NaN.
__device__ inline bool tile_cell_range(const Geom &g, const CellGrid &grid, const int32_t c0[3], const int32_t c1[3], double reach, int lo[3], int hi[3]) {
    double blo[3], bhi[3];
    crs_box_xyz(g, c0, c1, blo, bhi);
    bool any = grid.n_cells > 0;
    for (int q = 0; q < 3; ++q) {
        const double pad = reach * (1.0 + 1e-6) + 1e-9 * (fabs(blo[q]) + fabs(bhi[q]) + 1.0);
        const double fl = floor(((blo[q] - pad) - grid.lo[q]) / grid.edge), fh = floor(((bhi[q] + pad) - grid.lo[q]) / grid.edge);
        if (!(fh >= 0.0 && fl <= (double)(grid.dim[q] - 1))) any = false;
        lo[q] = fl < 0.0 ? 0 : (int)fmin(fl, (double)(grid.dim[q] - 1));
        hi[q] = fh > (double)(grid.dim[q] - 1) ? grid.dim[q] - 1 : (int)fmax(fh, 0.0);
    }
    return any;
}

// The points of the cells [lo, hi] streamed through a buffer of STAGE slots by a whole workgroup (uniform control flow: every thread walks the same
// rows and segments): load(slot, k) fills a slot from sorted position k, flush(n) works through the n slots filled -- behind a barrier of its own --
// whenever the buffer is full, and once more for what is left.  The report: the flushes, the slots of the last one when the buffer was not full
// then (else 0), the points in all.
struct StageReport { int runs, last; long long staged; };
template <int STAGE, typename Load, typename Flush>
__device__ inline StageReport stage_cell_rows(const CellGrid &g, const unsigned *__restrict__ start, const int lo[3], const int hi[3], Load load, Flush flush) {
    StageReport rep = {0, 0, 0};
    int fill = 0;
    for_each_cell_row(g, start, lo, hi, [&](unsigned b, const unsigned e) {
        rep.staged += (long long)(e - b);
        while (b < e) {
            const int take = (int)min((unsigned)(STAGE - fill), e - b);
            for (int i = threadIdx.x; i < take; i += 256) load(fill + i, b + (unsigned)i);
            fill += take; b += (unsigned)take;
            if (fill == STAGE) { flush(fill); ++rep.runs; __syncthreads(); fill = 0; }      // (the barrier: the buffer is written again)
        }
        return false;
    });
    if (fill > 0) { flush(fill); ++rep.runs; }
    rep.last = fill;
    return rep;
}
#endif  // __HIPCC__

}  // namespace pdbeda
