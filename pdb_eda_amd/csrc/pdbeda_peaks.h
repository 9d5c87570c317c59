// pdbeda_peaks.h -- density peak search: the local extrema of a map over the non-repeating box header.uniqueNcrs.
// No reference counterpart (the reference stops at blobs); the contract is spelled out at pdbeda_map_peaks in include/pdbeda.h.
//
//   k_peak_stencil   one pass over the grid: a tile of 64 x 8 x 8 voxels plus a one-voxel halo staged in LDS, the threshold test
//                    first, the 26 comparisons for the survivors only, the peaks of a wave row compacted by ballot / popcount
//                    into the tile's own segment of the plane's key arena.  Both signs in the same pass.  No global atomics:
//                    a counter every wave of the grid adds to costs ~12 ns an addition on this device (measured: 16 384 waves
//                    and 6 500 peaks, 255 us), so the slots of a tile are handed out by an LDS counter and the tile's count is stored.
//   k_peak_scan      one workgroup: the offsets of the tiles' segments in the compact list, the totals, the largest tile.
//   k_peak_finish    one thread per candidate: the key moves to its compact slot; crs, height, on_border, the three parabolas,
//                    the fractional crs -> xyz transform and the blob index out of a label volume.
//
// A candidate IS its 64-bit key: the high word holds the complement of the bits of |height| (non-negative floats order as
// their bits), the low word the c-major position (c * ur + r) * us + s.  Ascending keys = descending |height|, ties by c-major
// position: the order of the list.  Keys are unique, so the list does not depend on the order the atomics landed in.
#pragma once
#include "pdbeda_device.h"
#include "pdbeda_wave.h"

namespace pdbeda {

static constexpr int PK_SCAN_THREADS = 1024;

struct PeakCounters {
    unsigned long long tested[2];   // voxels that passed the threshold test, per plane
    unsigned long long peaks[2];    // peaks found, per plane (may exceed the plane's arena: then the job runs again)
    uint32_t max_tile[2];           // most peaks in one tile (may exceed the tiles' segments: then the job runs again)
    uint32_t pad[2];
};

struct PeakPlane {
    float cut;                      // float32 cutoff of the plane (inclusive)
    int32_t sign;                   // +1: maxima with D >= cut;  -1: minima with D <= cut
    unsigned long long cap;         // peaks the compact list (keys and columns) holds
    uint32_t seg;                   // keys a tile's segment holds
    uint32_t pad;
    unsigned long long *seg_keys;   // n_tiles x seg, in arrival order inside a tile
    uint32_t *tile_count;           // n_tiles: peaks found in the tile (all of them, stored or not)
    uint32_t *tile_tested;          // n_tiles: voxels of the tile that passed the threshold test
    uint32_t *tile_off;             // n_tiles: first compact slot of the tile's peaks
    unsigned long long *keys;       // the compact list
    // the finish kernel's columns, in arena (= arrival) order; the host applies the list order
    int32_t *crs;                   // cap x 3
    float *height;
    double *xyz;                    // cap x 3
    double *refined;
    int32_t *blob;
    uint8_t *border;
    const int32_t *labels;          // signed label volume [us][ur][uc] of the blob list given for this plane, or nullptr
};

struct PeakJobArgs {
    PeakPlane plane[2];
    int32_t n_planes;
    int32_t uc, ur, us;             // header.uniqueNcrs
    int32_t nc, nr;                 // stored row / section pitch (header.ncrs)
    int32_t n_tiles;
    PeakCounters *ctr;
};

__device__ inline unsigned long long peak_key(float v, uint32_t pos) {
    const uint32_t mag = __float_as_uint(v) & 0x7fffffffu;
    return ((unsigned long long)(~mag) << 32) | (unsigned long long)pos;
}

// Does the voxel (value v, sign sg) beat all of its neighbours inside the box?  tile: the LDS copy, (lc, lr, ls) the voxel's
// halo coordinates.  A neighbour LATER in c-major order is beaten on equality, an earlier one is not; a NaN on either side
// beats nothing (every comparison with it is false).
__device__ inline bool peak_beats_all(const float (*tile)[PK_HR][PK_HC], int lc, int lr, int ls, float v, int sg,
                                      int c, int r, int s, int uc, int ur, int us) {
    bool ok = true;
#pragma unroll
    for (int dc = -1; dc <= 1; ++dc) {
        if ((unsigned)(c + dc) >= (unsigned)uc) continue;
#pragma unroll
        for (int dr = -1; dr <= 1; ++dr) {
            if ((unsigned)(r + dr) >= (unsigned)ur) continue;
#pragma unroll
            for (int ds = -1; ds <= 1; ++ds) {
                if (dc == 0 && dr == 0 && ds == 0) continue;
                if ((unsigned)(s + ds) >= (unsigned)us) continue;
                const float nb = tile[ls + ds][lr + dr][lc + dc];
                const bool later = dc > 0 || (dc == 0 && (dr > 0 || (dr == 0 && ds > 0)));   // (compile-time per neighbour)
                const bool beats = sg > 0 ? (v > nb || (later && v == nb)) : (v < nb || (later && v == nb));
                ok = ok && beats;
            }
        }
    }
    return ok;
}

__global__ __launch_bounds__(PK_THREADS) void k_peak_stencil(PeakJobArgs a, const float *__restrict__ dens) {
    __shared__ float tile[PK_HS][PK_HR][PK_HC];
    __shared__ unsigned s_count[2], s_tested[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * PK_C, r0 = blockIdx.y * PK_R, s0 = blockIdx.z * PK_S;
    const int uc = a.uc, ur = a.ur, us = a.us;
    const unsigned tile_id = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const float no_voxel = __uint_as_float(0x7fc00000u);   // outside the box: never read by a comparison (the bounds tests above), NaN all the same
    if (threadIdx.x < 2) { s_count[threadIdx.x] = 0u; s_tested[threadIdx.x] = 0u; }
    halo_stage<float>(tile, dens, a.nc, a.nr, c0, r0, s0, uc, ur, us, no_voxel);
    __syncthreads();
    const int c = c0 + lane;
    unsigned tested[2] = {0u, 0u};
    for (int q = wave; q < PK_R * PK_S; q += PK_THREADS / 64) {
        const int ss = q / PK_R, rr = q - ss * PK_R;
        const int r = r0 + rr, s = s0 + ss;
        if (r >= ur || s >= us) continue;                 // wave-uniform
        const float v = tile[ss + 1][rr + 1][lane + 1];
        const bool in = c < uc;
#pragma unroll
        for (int p = 0; p < 2; ++p) {                     // (unrolled: the planes stay kernel arguments, not a scratch copy)
            if (p >= a.n_planes) break;
            const PeakPlane &pl = a.plane[p];
            const bool pass = in && (pl.sign > 0 ? v >= pl.cut : v <= pl.cut);
            const unsigned long long passed = __ballot(pass);
            if (passed == 0ull) continue;                 // wave-uniform: most rows at 3 sigma
            tested[p] += (unsigned)__popcll(passed);      // (the same number in every lane; lane 0 reports it)
            const bool peak = pass && peak_beats_all(tile, lane + 1, rr + 1, ss + 1, v, pl.sign, c, r, s, uc, ur, us);
            const unsigned long long found = __ballot(peak);
            if (found == 0ull) continue;
            unsigned base = 0u;
            if (lane == 0) base = atomicAdd(&s_count[p], (unsigned)__popcll(found));
            base = __shfl(base, 0);
            if (peak) {
                const unsigned slot = base + (unsigned)__popcll(found & ((1ull << lane) - 1ull));
                if (slot < pl.seg)                        // (beyond the segment: counted, not stored -- the job runs again)
                    pl.seg_keys[(unsigned long long)tile_id * pl.seg + slot] = peak_key(v, (uint32_t)(((int64_t)c * ur + r) * us + s));
            }
        }
    }
    if (lane == 0) {
        if (tested[0]) atomicAdd(&s_tested[0], tested[0]);
        if (tested[1]) atomicAdd(&s_tested[1], tested[1]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p >= a.n_planes) break;
            a.plane[p].tile_count[tile_id] = s_count[p];
            a.plane[p].tile_tested[tile_id] = s_tested[p];
        }
    }
}

// The compact slots of the tiles' peaks: an exclusive scan of min(count, segment) over the tiles, one workgroup; the totals
// (every peak found, stored or not), the tested voxels and the fullest tile go to the counters.
__global__ __launch_bounds__(PK_SCAN_THREADS) void k_peak_scan(PeakJobArgs a) {
    __shared__ unsigned long long s_sum[PK_SCAN_THREADS];
    __shared__ unsigned long long s_all[PK_SCAN_THREADS], s_test[PK_SCAN_THREADS];
    __shared__ unsigned s_max[PK_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (a.n_tiles + PK_SCAN_THREADS - 1) / PK_SCAN_THREADS;
    const int lo = min(t * per, a.n_tiles), hi = min(lo + per, a.n_tiles);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p >= a.n_planes) break;
        const PeakPlane &pl = a.plane[p];
        unsigned long long kept = 0ull, all = 0ull, test = 0ull;
        unsigned most = 0u;
        for (int i = lo; i < hi; ++i) {
            const unsigned n = pl.tile_count[i];
            kept += n < pl.seg ? n : pl.seg;
            all += n;
            test += pl.tile_tested[i];
            most = n > most ? n : most;
        }
        s_sum[t] = kept; s_all[t] = all; s_test[t] = test; s_max[t] = most;
        __syncthreads();
        for (int d = 1; d < PK_SCAN_THREADS; d <<= 1) {          // inclusive scan of the kept counts; plain sums of the rest
            const unsigned long long add = t >= d ? s_sum[t - d] : 0ull;
            const unsigned long long add_all = t + d < PK_SCAN_THREADS && (t & (2 * d - 1)) == 0 ? s_all[t + d] : 0ull;
            const unsigned long long add_test = t + d < PK_SCAN_THREADS && (t & (2 * d - 1)) == 0 ? s_test[t + d] : 0ull;
            const unsigned other = t + d < PK_SCAN_THREADS && (t & (2 * d - 1)) == 0 ? s_max[t + d] : 0u;
            __syncthreads();
            s_sum[t] += add; s_all[t] += add_all; s_test[t] += add_test; s_max[t] = other > s_max[t] ? other : s_max[t];
            __syncthreads();
        }
        unsigned long long off = s_sum[t] - kept;                // exclusive
        for (int i = lo; i < hi; ++i) {
            const unsigned n = pl.tile_count[i];
            pl.tile_off[i] = (uint32_t)off;
            off += n < pl.seg ? n : pl.seg;
        }
        if (t == 0) {
            a.ctr->peaks[p] = s_all[0];
            a.ctr->tested[p] = s_test[0];
            a.ctr->max_tile[p] = s_max[0];
        }
        __syncthreads();
    }
}

// One parabola through (-1, lo), (0, v), (+1, hi): the offset of its vertex, clamped to half a voxel; 0 when the parabola is
// flat or the voxel has no neighbour on either side along the axis.  *term = (lo - hi) * offset, the axis' share of the refined height.
__device__ inline double peak_parabola(bool have_both, double lo, double v, double hi, double *term) {
    *term = 0.0;
    if (!have_both) return 0.0;
    const double den = (lo - 2.0 * v) + hi;
    if (den == 0.0) return 0.0;
    double off = (0.5 * (lo - hi)) / den;
    off = off < -0.5 ? -0.5 : (off > 0.5 ? 0.5 : off);
    *term = (lo - hi) * off;
    return off;
}

__global__ __launch_bounds__(256) void k_peak_finish(PeakJobArgs a, const float *__restrict__ dens, const Geom *__restrict__ geom) {
    const Geom &g = *geom;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p >= a.n_planes) break;
        const PeakPlane &pl = a.plane[p];
        const int64_t slots = (int64_t)a.n_tiles * pl.seg;
        for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (int64_t)gridDim.x * blockDim.x) {
            const int64_t t = j / pl.seg;
            const uint32_t k = (uint32_t)(j - t * pl.seg), n = pl.tile_count[t];
            if (k >= (n < pl.seg ? n : pl.seg)) continue;
            const unsigned long long i = (unsigned long long)pl.tile_off[t] + k;
            if (i >= pl.cap) continue;                       // (the compact list is sized for every segment full: a job that ran again, for its count)
            const unsigned long long key = pl.seg_keys[j];
            pl.keys[i] = key;
            const uint32_t pos = (uint32_t)(key & 0xffffffffull);
            const int32_t s = (int32_t)(pos % (uint32_t)a.us), cr = (int32_t)(pos / (uint32_t)a.us);
            const int32_t r = cr % a.ur, c = cr / a.ur;
            const int64_t at = ((int64_t)s * a.nr + r) * a.nc + c;
            const float vf = dens[at];
            const double v = (double)vf;
            const bool c_in = c > 0 && c + 1 < a.uc, r_in = r > 0 && r + 1 < a.ur, s_in = s > 0 && s + 1 < a.us;
            double tc, tr, ts;
            const double oc = peak_parabola(c_in, c_in ? (double)dens[at - 1] : 0.0, v, c_in ? (double)dens[at + 1] : 0.0, &tc);
            const double orr = peak_parabola(r_in, r_in ? (double)dens[at - a.nc] : 0.0, v, r_in ? (double)dens[at + a.nc] : 0.0, &tr);
            const int64_t sec = (int64_t)a.nr * a.nc;
            const double os = peak_parabola(s_in, s_in ? (double)dens[at - sec] : 0.0, v, s_in ? (double)dens[at + sec] : 0.0, &ts);
            const double sum = (tc + tr) + ts;
            const double frac[3] = {(double)c + oc, (double)r + orr, (double)s + os};
            double xyz[3];
            crs2xyz_frac(g, frac, xyz);
            pl.crs[3 * i + 0] = c; pl.crs[3 * i + 1] = r; pl.crs[3 * i + 2] = s;
            pl.height[i] = vf;
            pl.xyz[3 * i + 0] = xyz[0]; pl.xyz[3 * i + 1] = xyz[1]; pl.xyz[3 * i + 2] = xyz[2];
            pl.refined[i] = v - 0.25 * sum;
            pl.border[i] = (c_in && r_in && s_in) ? 0 : 1;
            int32_t blob = -1;
            if (pl.labels) {
                const int32_t lab = pl.labels[((int64_t)s * a.ur + r) * a.uc + c];
                blob = pl.sign > 0 ? (lab > 0 ? lab - 1 : -1) : (lab < 0 ? -lab - 1 : -1);
            }
            pl.blob[i] = blob;
        }
    }
}

}  // namespace pdbeda
