/*
 * pdbeda.h -- C-ABI of libpdbeda_hip.so: the MI355X (gfx950) electron-density voxel core.
 *
 * This is the drop-in boundary for the one accelerated path of pdb_eda: everything the
 * reference routes through its `utils` seam (`from . import cutils as utils`,
 * /root/reference/pdb_eda/ccp4.py:16-19 and densityAnalysis.py:26-29).  A per-voxel
 * Python-tuple API cannot cross a device boundary, so the seam sits one level up:
 * ccp4.py hands over the raw [s][r][c] grid and the unit-cell basis once
 * (pdbeda_map_upload) and each entry point below replaces one reference call chain,
 * cited per function (paths relative to /root/reference/pdb_eda/).
 *
 * Conventions
 *   - plain C types only; all functions return 0 on success or a negative pdbeda_status;
 *     pdbeda_last_error(ctx) gives the message.  No exception crosses the ABI.
 *   - the caller owns every host buffer; the library owns device memory behind the
 *     opaque handles.  A context is bound to ONE device and ONE HIP stream; N contexts
 *     = N streams.  Calls on one context are not re-entrant; different contexts may be
 *     used from different threads concurrently.
 *   - crs triples are (column, row, section) = the reference's crsCoord order.
 *   - "cutoff"/"radius" parameters are C floats on purpose: the reference's Cython
 *     declares them `float` (cutils.pyx:28,185,205,220,250,273), i.e. the Python double
 *     is rounded to float32 before use.
 *   - there is no CPU fallback: without a usable gfx950 device every entry point fails
 *     with PDBEDA_ERR_DEVICE.
 */
#ifndef PDBEDA_H
#define PDBEDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pdbeda_status {
    PDBEDA_OK = 0,
    PDBEDA_ERR_DEVICE = -1,   /* no device / HIP runtime error */
    PDBEDA_ERR_ARGUMENT = -2, /* bad argument */
    PDBEDA_ERR_MEMORY = -3,   /* device or host allocation failed */
    PDBEDA_ERR_CAPACITY = -4, /* caller buffer too small */
    PDBEDA_ERR_STATE = -5,    /* handle used in the wrong state */
    PDBEDA_ERR_TIMEOUT = -6   /* the per-entry watchdog expired; the context is abandoned (see pdbeda_ctx_set_timeout) */
} pdbeda_status;

typedef struct pdbeda_ctx pdbeda_ctx;           /* device + stream + reusable workspace */
typedef struct pdbeda_map pdbeda_map;           /* one density grid resident in HBM */
typedef struct pdbeda_bloblist pdbeda_bloblist; /* result of a labelling call */
typedef struct pdbeda_peaklist pdbeda_peaklist; /* result of a peak search */

/* The "unit-cell basis" ccp4.py computes on the host (DensityHeader, ccp4.py:225-286). */
typedef struct pdbeda_geometry {
    int32_t ncrs[3];         /* header.ncrs                                   ccp4.py:168   */
    int32_t crs_start[3];    /* header.crsStart                               ccp4.py:186   */
    int32_t xyz_interval[3]; /* header.xyzInterval                            ccp4.py:227   */
    int32_t map2xyz[3];      /* header.map2xyz                                ccp4.py:230-234 */
    int32_t map2crs[3];      /* header.map2crs                                ccp4.py:235   */
    int32_t orthogonal;      /* alpha == beta == gamma == 90                  ccp4.py:297   */
    double ortho[9];         /* header.orthoMat (row major)                   ccp4.py:248-250 */
    double deortho[9];       /* header.deOrthoMat (row major)                 ccp4.py:252-253 */
    double origin[3];        /* header.origin                                 ccp4.py:272-286 */
    double grid_len[3];      /* header.gridLength                             ccp4.py:228   */
    double unit_volume;      /* header.unitVolume                             ccp4.py:243-244 */
} pdbeda_geometry;

/* ---- library / context ------------------------------------------------------------ */
const char *pdbeda_version(void);
int pdbeda_device_count(void);
/* PCI address of a device ("0000:dc:00.0"): /sys/bus/pci/devices/<address>/local_cpulist names the host cores of the GPU's
 * NUMA node.  The reference's multiprocessing pool (multipleStructures.py:167-168) leaves placement to the OS; a worker that
 * feeds a GPU from the other socket reads and uploads its maps across the socket link (measured: 4x slower per entry). */
int pdbeda_device_pci_address(int device_id, char *out, int out_len);
int pdbeda_ctx_create(int device_id, pdbeda_ctx **out);
/* Bind to an existing hipStream_t (e.g. torch's current stream); stream == NULL -> new stream. */
int pdbeda_ctx_create_on_stream(int device_id, void *hip_stream, pdbeda_ctx **out);
/* Waits for the stream and releases the context's device memory; arenas that live handles of the caller still hold stay
 * theirs.  PDBEDA_ERR_STATE (everything is released all the same): no handle of the context is alive and one of its arenas is
 * still lent -- the library itself lost it.  With live handles the status says nothing about arenas. */
int pdbeda_ctx_destroy(pdbeda_ctx *ctx);
int pdbeda_ctx_synchronize(pdbeda_ctx *ctx);
void *pdbeda_ctx_stream(pdbeda_ctx *ctx); /* the hipStream_t the kernels are launched on */
/* Per-entry watchdog: the reference wraps every entry of `pdb_eda multiple` in a SIGALRM time-out
 * (multipleStructures.py:297-304, 359-377), which threads cannot use.  With seconds > 0 every wait of this context on its
 * stream is a timed hipStreamQuery loop against ONE deadline, now + seconds, shared by all waits until the next call of this
 * function: the caller re-arms it when an entry starts (an entry makes dozens of waits; a clock per wait would let it run for
 * many multiples of the time-out).  When the deadline passes the call returns PDBEDA_ERR_TIMEOUT, the context is marked
 * abandoned (every later call on it or its handles fails at once with the same status) and pdbeda_ctx_destroy does not wait
 * for the stream: the context is parked and its device memory -- pool, buffers, and the arenas of the maps / jobs the entry
 * left behind -- is released by pdbeda_reap_abandoned once the stream has drained.  seconds == 0 disarms the watchdog (plain
 * hipStreamSynchronize).  Host-side phases of an entry are outside the library: the caller checks its own clock. */
int pdbeda_ctx_set_timeout(pdbeda_ctx *ctx, double seconds);
/* Destroy the abandoned contexts of this process whose streams have drained (hipStreamQuery, no waiting); returns how many are
 * still parked.  Called by the library itself at every context creation and before an allocation is reported as failed (then
 * the parked arenas of the sibling contexts on the device go back to the driver too); exposed for callers and tests. */
int64_t pdbeda_reap_abandoned(void);
const char *pdbeda_last_error(pdbeda_ctx *ctx);
/* Per-kernel timing with HIP events recorded on the context's stream (measurement aid for
 * bench.py; no reference counterpart).  profile_end synchronises and writes one
 * "kernel_name calls total_ms" line per kernel into buf (and a "host_peak_sort" line when peak lists were ordered meanwhile:
 * host time, the same units). */
int pdbeda_ctx_profile_begin(pdbeda_ctx *ctx);
int pdbeda_ctx_profile_end(pdbeda_ctx *ctx, char *buf, int64_t cap);

/* ---- map residency: replaces DensityMatrix.__init__ (ccp4.py:322-341) ------------- */
/* density: host float32 [ns][nr][nc] (c fastest); copied to HBM. */
int pdbeda_map_upload(pdbeda_ctx *ctx, const float *density, const pdbeda_geometry *geom, pdbeda_map **out);
/* ... with the map's mean / std from the same wait (see pdbeda_map_upload_file_stats); mean / std may be NULL. */
int pdbeda_map_upload_stats(pdbeda_ctx *ctx, const float *density, const pdbeda_geometry *geom, pdbeda_map **out, double *mean, double *std);
/* density_dev: a device pointer the caller keeps alive (zero-copy, e.g. a torch tensor). */
int pdbeda_map_from_device(pdbeda_ctx *ctx, const float *density_dev, const pdbeda_geometry *geom, pdbeda_map **out);
/* The caller has rewritten a borrowed buffer in place: drop what the library cached about the map's contents (the quantum of
 * the order-independent blob sums, derived once per map from sum |rho| and max |rho|).  The reference has no counterpart: its
 * DensityMatrix owns its array (ccp4.py:322-341).  A map that holds a NaN or an infinity is refused by the labelling calls. */
int pdbeda_map_invalidate(pdbeda_map *map);
/* The grid of a CCP4 FILE straight into HBM (ccp4.read -> parse, ccp4.py:58-127): n = ncrs[0]*ncrs[1]*ncrs[2] float32 values
 * starting at byte `offset` (1024 + the symmetry records) of `path`, read through the process's upload engine (three pread() readers with
 * pinned chunks of their own, their PCIe copies queued on three streams; the context's stream is ordered behind them); byteswap != 0 when the
 * file has the other endianness (swapped on the device).  No host copy
 * of the map exists afterwards (pdbeda_map_download fetches one on demand). */
int pdbeda_map_upload_file(pdbeda_ctx *ctx, const char *path, int64_t offset, int byteswap, const pdbeda_geometry *geom, pdbeda_map **out);
/* The same with the map's mean and standard deviation (pdbeda_map_stats: DensityMatrix.meanDensity / stdDensity, ccp4.py:343-361)
 * computed behind the copies and returned from the SAME wait: every cutoff of the analysis is mean + k std, so the statistics are
 * what a caller asks for next.  mean / std may be NULL. */
int pdbeda_map_upload_file_stats(pdbeda_ctx *ctx, const char *path, int64_t offset, int byteswap, const pdbeda_geometry *geom, pdbeda_map **out,
                                 double *mean, double *std);
int pdbeda_map_free(pdbeda_map *map);
/* A new map on the geometry of `a` with density  float32( double(a) + alpha * double(b) )  per voxel -- the Fc map of
 * DensityAnalysis.fc is (2Fo-Fc) - 2 (Fo-Fc), densityAnalysis.py:426-435 (alpha = -2).  Same grid shape required.
 * The product and the sum are two fp64 roundings (no fused multiply-add) and the result is rounded to nearest float32 once:
 * numpy's bits, float32 subnormals in and out included, and a sum beyond the float32 range becomes an infinity. */
int pdbeda_map_combine(pdbeda_map *a, pdbeda_map *b, double alpha, pdbeda_map **out);
/* One digit of a radix select over the voxels of the unique box with |a| < cut_a and |a + alpha b| < cut_b (b may be NULL:
 * then only the first test applies and which must be 0): the 65536-bin histogram of bits [shift, shift+16) of the key of the
 * voxels whose key agrees with `prefix` on `prefix_mask`.  key = bits of float |a| (which = 0, 32 bits) or of double
 * |a + alpha b| (which = 1, 64 bits) -- both orders are the numeric orders.  Host code walks the digits to an exact order
 * statistic: DensityAnalysis.medianAbsFoFc (densityAnalysis.py:783-801) without moving the maps.  hist: 65536 uint32.
 * Both tests are strict `<` on fp64 magnitudes: a voxel exactly on a cut is excluded, and so is one whose a or a + alpha b is a
 * NaN or an infinity (cut_a = cut_b = inf keeps every voxel whose two magnitudes are finite).  +0 and -0 have one key (0);
 * subnormal values are kept as they are, with keys of their own.  shift: 0 to 48. */
int pdbeda_abs_select_hist(pdbeda_map *a, pdbeda_map *b, double alpha, double cut_a, double cut_b, int which, int shift,
                           unsigned long long prefix, unsigned long long prefix_mask, uint32_t *hist);
/* Copy the float32 grid [ns][nr][nc] back to the host (inspection; DensityMatrix.density of a derived map). */
int pdbeda_map_download(pdbeda_map *map, float *density_out);

/* ---- whole-map reductions --------------------------------------------------------- */
/* DensityMatrix.meanDensity / stdDensity: np.mean / np.std (population) over ALL stored
 * voxels in fp64 (ccp4.py:343-363). */
int pdbeda_map_stats(pdbeda_map *map, double *mean, double *std);
/* utils.sumOfAbs via getTotalAbsDensity: sum |v| for |v| > cutoff, strict (cutils.pyx:28-39,
 * ccp4.py:365-376).  The cutoff is a float32: a caller that holds a double rounds it to nearest first, and
 * the comparison is then made on the exact values.  A NaN voxel is greater than nothing and is skipped; an infinite one makes
 * the sum infinite.  Summed in fp64 in a fixed order: the same map and cutoff give the same bits in every run. */
int pdbeda_sum_of_abs(pdbeda_map *map, float cutoff, double *out);

/* ---- point / geometry helpers (batched) ------------------------------------------- */
/* utils.getPointDensityFromCrs (cutils.pyx:125-145): periodic wrap, 0 outside the data. */
int pdbeda_point_density(pdbeda_map *map, const int32_t *crs, int64_t n, double *out);
/* utils.testValidCrs (cutils.pyx:147-167). */
int pdbeda_valid_crs(pdbeda_map *map, const int32_t *crs, int64_t n, uint8_t *out);
/* DensityHeader.crs2xyzCoord / xyz2crsCoord evaluated by the DEVICE code (ccp4.py:288-316);
 * exposed so the parity tests can pin the kernels' geometry arithmetic. */
int pdbeda_crs2xyz(pdbeda_map *map, const int32_t *crs, int64_t n, double *xyz);
int pdbeda_xyz2crs(pdbeda_map *map, const double *xyz, int64_t n, int32_t *crs);

/* ---- blob labelling --------------------------------------------------------------- */
#define PDBEDA_FLAG_LABELS 1u /* also materialise the dense int32 label volume in HBM */

/* DensityMatrix.createFullBlobList(cutoff) = utils.createFullCrsList + utils.createCrsLists
 * + DensityBlob.fromCrsList (ccp4.py:463-485, 522-545; cutils.pyx:185-203, 44-70):
 * inclusive threshold over the non-repeating box header.uniqueNcrs, 26-connected
 * components (non-periodic), per-blob fp64 statistics, blobs ordered by the c-major
 * position of their first voxel (the reference's emission order).  Asynchronous: returns
 * after enqueueing; the first accessor synchronises.  cutoff == 0 -> PDBEDA_ERR_ARGUMENT
 * (the reference returns None). */
int pdbeda_full_blobs(pdbeda_map *map, float cutoff, uint32_t flags, pdbeda_bloblist **out);
/* Fused green/red: ONE pass over the grid labels density >= cutoff_pos and
 * density <= cutoff_neg (densityAnalysis.py:392-412 calls the above twice). */
int pdbeda_full_blobs_pm(pdbeda_map *map, float cutoff_pos, float cutoff_neg, uint32_t flags,
                         pdbeda_bloblist **green, pdbeda_bloblist **red);

/* DensityMatrix.findAberrantBlobs (ccp4.py:437-461) = utils.getSphereCrsFromXyz[List]
 * (cutils.pyx:220-271) + createBlobList, batched: atoms [group_offsets[g], group_offsets[g+1])
 * form group g whose sphere voxels are unioned on RAW crs (a one-atom group is the
 * single-coordinate call).  xyz: n_atoms x 3 doubles (float32 atom coordinates promoted
 * exactly); radii: per atom.  Blobs come back sorted by (group, c-major first voxel of the
 * group's bounding box).
 * A non-finite coordinate or radius: PDBEDA_ERR_ARGUMENT, the message names the atom, before anything is staged or launched; the
 * context stays usable.  A finite coordinate or radius beyond what the host may turn into grid indices (an index or a box
 * half-width of 2^29 grid steps or more, a negative radius) is not refused: the device sizes that batch itself, behind one more
 * wait, as it sizes voxel lists. */
int pdbeda_sphere_blobs(pdbeda_map *map, const double *xyz, const float *radii, int64_t n_atoms,
                        const int64_t *group_offsets, int64_t n_groups, float density_cutoff,
                        pdbeda_bloblist **out);

/* DensityMatrix.createBlobList(crsList) (ccp4.py:475-485) on explicit raw voxel sets:
 * voxels [group_offsets[g], group_offsets[g+1]) of crs (n x 3) form group g (duplicates
 * collapse, as in DensityBlob's set; voxels that are periodic images of each other stay
 * distinct: connectivity is on raw crs).  A group may be empty and then has no blob.  Blobs
 * come back sorted by (group, first_key), first_key strictly increasing inside a group: the
 * order of pdbeda_sphere_blobs.  Used for DensityBlob.merge / fromCrsList and for
 * the residue / domain cloud unions of aggregateCloud (densityAnalysis.py:646-708). */
int pdbeda_list_blobs(pdbeda_map *map, const int32_t *crs, int64_t n, const int64_t *group_offsets,
                      int64_t n_groups, pdbeda_bloblist **out);

/* ---- blob list accessors ---------------------------------------------------------- */
int64_t pdbeda_bloblist_count(pdbeda_bloblist *bl);      /* number of blobs (synchronises) */
int64_t pdbeda_bloblist_num_voxels(pdbeda_bloblist *bl); /* total voxels in all blobs */
/* Per blob, any pointer may be NULL: n voxels, totalDensity, centroid[3], coordCenter[3],
 * volume (= unitVolume * n), first_key (c-major position of the first voxel), group. */
int pdbeda_bloblist_stats(pdbeda_bloblist *bl, int64_t *n, double *total_density, double *centroid,
                          double *coord_center, double *volume, int64_t *first_key, int32_t *group);
/* Voxel membership: crs (N x 3, raw coordinates) grouped by blob in blob order;
 * blob_offsets has count+1 entries. */
int pdbeda_bloblist_voxels(pdbeda_bloblist *bl, int32_t *crs, int64_t *blob_offsets);
/* The shape of every blob (no reference counterpart: a reference blob knows its voxel count, total density and two centres, and
 * nothing about its extent, its elongation or its strongest voxel).  Works on every kind of list (whole-map, either list of a fused
 * _pm call, pdbeda_sphere_blobs, pdbeda_list_blobs); rows in the list's blob order, the order of pdbeda_bloblist_stats; any output
 * pointer may be NULL.  Synchronous.
 * A voxel's density is utils.getPointDensityFromCrs of its raw crs (periodic wrap, 0 where nothing is stored: the density of the
 * blob sums); w = |density|.  Per blob:
 *   box_lo[3], box_hi[3]   the smallest and the largest raw c, r, s over the blob's voxels (inclusive);
 *   extreme_crs[3], extreme   the voxel with the largest w and its signed value; among voxels of equal w the one that comes first in
 *                          (c, r, s) order of raw crs, c most significant (the c-major order of the peaks): a strict total order, so
 *                          the answer does not depend on the order of the voxel list;
 *   s1[3], s2[6]           exact integer sums of the offsets d = crs - box_lo: sum d_c, d_r, d_s and sum d_c d_c, d_c d_r, d_c d_s,
 *                          d_r d_r, d_r d_s, d_s d_s;
 *   sw, sw1[3], sw2[6]     the same sums weighted by w: sum w, sum w d, sum w d d'.  w is rounded once to the map's fixed-point quantum
 *                          (the quantum of the blob sums: <= 2^-36 max |rho|), the products with the integer offsets are taken exactly
 *                          and the sums are folded as integers and converted once: bit-identical from run to run, within
 *                          quantum / 2 * d d' per voxel of the exact sum (d d' = 1 for sw).  A one-voxel blob has exact zeros in s1, s2,
 *                          sw1 and sw2.
 * Central moments, the conversion to Angstrom and the principal axes are the caller's (a few fp64 operations per row).
 * A list with no blobs succeeds and touches nothing.  PDBEDA_ERR_ARGUMENT: a NULL or freed list; a list that holds a blob whose box is
 * 2^15 voxels or more wide along an axis (found by the first of the two passes, before any moment is summed); a sphere / list batch of
 * 2^24 voxels or more, any list of 2^31 voxels or more (what the integer accumulators hold).  The rows are kept with the list: a second call copies them without a launch.  A failing call leaves the
 * context usable. */
int pdbeda_bloblist_moments(pdbeda_bloblist *bl, int32_t *box_lo, int32_t *box_hi, int32_t *extreme_crs, float *extreme,
                            int64_t *s1, int64_t *s2, double *sw, double *sw1, double *sw2);
/* Dense labels of a full-map list: int32 [us][ur][uc] over header.uniqueNcrs, blob index or
 * -1.  Computed on first use unless PDBEDA_FLAG_LABELS was given. */
int pdbeda_bloblist_labels(pdbeda_bloblist *bl, int32_t *labels_host);
/* For every blob of list a, the nearest blob of list b in the sense of a caller-made table of voxel offsets (no reference counterpart: a
 * reference blob knows nothing about any other blob).  The contract is purely integer.
 * a and b are whole-map lists of the same context whose maps have the same header.uniqueNcrs: the green and the red list of one fused _pm
 * call, two separately labelled lists of one map, or lists of two maps on one grid.  offsets (n_offsets x 3: dc, dr, ds) is an ORDERED
 * neighbourhood table; the library gives it no geometric meaning and does not check its order.  Per blob i of a, over all pairs (p, t) with
 * p a voxel of blob i and p + offsets[t] inside the non-repeating box header.uniqueNcrs (nothing wraps, as in the peaks) and a voxel of some
 * blob of b: the smallest t, and among the voxels p with that t the one that comes first in c-major (c, r, s) order, c most significant
 * (the order of first_key in pdbeda_bloblist_stats) -- a strict total order, so the answer does not depend on the order of the voxel
 * list or of any atomic.  index[i] = t, voxel[i] = p, partner_voxel[i] = p + offsets[t], partner[i] = the index in b of the blob that
 * holds that voxel; without a pair index and partner are -1 and the two voxels 0.  The offset (0, 0, 0) is legal (it hits where lists of
 * two maps overlap).
 * Any output pointer may be NULL.  Synchronous; rows in the blob order of a, the order of pdbeda_bloblist_stats.  An empty a or b, or
 * n_offsets == 0, succeeds with rows of -1 and launches no search.  PDBEDA_ERR_ARGUMENT (nothing has been launched): a NULL or freed
 * list; a == b; lists of different contexts; a list that is not whole-map; unequal uniqueNcrs; n_offsets > 16384 or < 0; an offset
 * component outside [-127, 127] (the table lives in LDS as packed words).  PDBEDA_ERR_TIMEOUT on a context whose watchdog has expired.
 * A failing call leaves the context usable. */
int pdbeda_bloblist_nearest(pdbeda_bloblist *a, pdbeda_bloblist *b, const int32_t *offsets, int64_t n_offsets, int32_t *index,
                            int32_t *partner, int32_t *voxel, int32_t *partner_voxel);
int pdbeda_bloblist_free(pdbeda_bloblist *bl);
/* Diagnostic (no reference counterpart): counters of the labelling job behind a list,
 * out[8] = run ids, component ids, runs of the job beyond the first (1 = the typical-size arena was too small for this map and
 * the job ran again in a worst-case one), blobs, tiles off the fast path by kind (unit tiles: run slots full; wide tiles: more
 * components than the LDS tables hold, united in LDS all the same; unit tiles: no ids left for a wide tile), bytes of device memory
 * the job holds. */
int pdbeda_bloblist_counters(pdbeda_bloblist *bl, int64_t *out);

/* ---- density peaks ---------------------------------------------------------------- */
/* The local extrema of a map (no reference counterpart: the reference stops at blobs, whose centroid is the wrong handle on a
 * blob that covers two waters).  Domain: the voxels of the non-repeating box header.uniqueNcrs (the domain of
 * createFullCrsList, utils.py:180-198); the neighbourhood of a voxel is those of its 26 neighbours that lie inside that box
 * (nothing wraps: the connectivity of createCrsLists).  For cutoff > 0 voxel a BEATS voxel b when D[a] > D[b], or D[a] == D[b]
 * and a comes first in c-major (c, r, s) order; for cutoff < 0 the same with <: a strict total order, so plateaus have exactly
 * one peak.  A PEAK is a voxel with D >= cutoff (D <= cutoff for cutoff < 0; inclusive, float32 cutoff) that beats every
 * neighbour; a NaN voxel is never a peak and beats nothing.  Per peak: crs (raw, as pdbeda_bloblist_voxels), height (the
 * voxel value), on_border (fewer than 26 neighbours in the box), and a position / height refined by one parabola per axis in
 * fp64: with a, v, b the values at -1, 0, +1 along the axis and den = a - 2 v + b, offset = 0.5 (a - b) / den, taken as 0 when
 * den == 0 or an axial neighbour is outside the box, clamped to [-0.5, 0.5]; refined_height = v - 0.25 sum over axes of
 * (a - b) offset; refined_xyz = crs2xyzCoord (ccp4.py:304-316) of the fractional crs.  The list is ordered by descending
 * |height|, ties by c-major position, bit-identical from run to run.
 * blobs: NULL, or the whole-map list of the SAME map and float32 cutoff (else PDBEDA_ERR_ARGUMENT; the call then waits for the
 * labelling job): a peak passes the cutoff, so it lies in exactly one blob of that list -- `blob` is its index there (-1
 * throughout without a list).  The blob list must stay alive until the first accessor of the peak list has returned.
 * cutoff == 0 -> PDBEDA_ERR_ARGUMENT.  Asynchronous: returns after enqueueing; the first accessor synchronises. */
int pdbeda_map_peaks(pdbeda_map *map, float cutoff, pdbeda_bloblist *blobs /* may be NULL */, pdbeda_peaklist **out);
/* Fused: ONE pass over the grid finds the maxima with D >= cutoff_pos and the minima with D <= cutoff_neg (the green and red
 * peaks of an Fo-Fc map, as pdbeda_full_blobs_pm does for blobs); each list equals the single call's to the bit.  No reference
 * counterpart.  Asynchronous until the first accessor of either list. */
int pdbeda_map_peaks_pm(pdbeda_map *map, float cutoff_pos, float cutoff_neg,
                        pdbeda_bloblist *green, pdbeda_bloblist *red /* both may be NULL */,
                        pdbeda_peaklist **pos, pdbeda_peaklist **neg);
/* Number of peaks (no reference counterpart; synchronises, orders the list, and runs the job again when its typical-size
 * arena -- room for a peak per 64 voxels of every 64 x 8 x 8 tile -- was too small for this map). */
int64_t pdbeda_peaklist_count(pdbeda_peaklist *pl);
/* The columns of the list in list order (no reference counterpart; synchronises): crs n x 3, height n, refined_xyz n x 3,
 * refined_height n, blob n, on_border n. */
int pdbeda_peaklist_rows(pdbeda_peaklist *pl, int32_t *crs, float *height, double *refined_xyz,
                         double *refined_height, int32_t *blob, uint8_t *on_border);   /* any pointer may be NULL */
/* Diagnostic (no reference counterpart; synchronises), like pdbeda_bloblist_counters: out[4] = candidates tested (voxels of
 * the box that pass the cutoff), peaks, runs of the job beyond the first (1 = the typical-size arena overflowed), bytes of
 * device memory the job holds. */
int pdbeda_peaklist_counters(pdbeda_peaklist *pl, int64_t *out);
/* Peak basins (no reference counterpart): the significant voxels divided among the peaks of the list by steepest ascent, with
 * per-basin sums and the highest pass to an adjacent basin.  pl: a list of pdbeda_map_peaks or either list of
 * pdbeda_map_peaks_pm; its map, sign and float32 cutoff are the job's.  The MAP MUST STILL BE ALIVE AND UNCHANGED since the peak
 * call (the list keeps a pointer to it, not a copy).  Rows come in the list's order.
 * Domain: the significant voxels of the non-repeating box header.uniqueNcrs, D >= cutoff (D <= cutoff for a negative cutoff;
 * inclusive, a NaN fails): exactly the candidates of the peak search.  Neighbours are the 26 neighbours inside the box; nothing wraps.
 * The PARENT of a significant voxel v is the voxel, among v and its significant neighbours, that BEATS all the others in the
 * sense of pdbeda_map_peaks (greater |D|; on equal |D| the one that comes first in c-major (c, r, s) order).  A voxel that is its
 * own parent is a ROOT; the root of v is reached by following parents (the order is strict: the walk ends and is unique); the
 * BASIN of peak i is every significant voxel whose root is peak i's voxel.  On a map without NaN the roots are the peaks.  A root
 * that is not in the list can only sit beside a NaN voxel (which the peak rule lets nothing beat): its voxels are ORPHANS, enter
 * no row, carry -1 in `basin` and are counted in `counters`.
 * Per peak i:
 *   n          voxels of the basin (>= 1: the peak itself);
 *   sum        their density: each voxel rounded once to the map's fixed-point quantum (the quantum of the blob sums, as in
 *              pdbeda_map_partition), folded as integers and converted once -- bit-identical from run to run, within quantum / 2
 *              per voxel of the exact sum.  A non-finite voxel is counted in n and s1 and enters neither sum nor sw1;
 *   s1[3]      exact integer sums of d = crs - crs(peak i);
 *   sw1[3]     sum of w d with w = |density| rounded to the same quantum; the products are exact and folded as integers.  (The
 *              sum of w is |sum|: all voxels of a basin have the cutoff's sign.)  A one-voxel basin has exact zeros in s1 and sw1;
 *   saddle, neighbour   over all pairs (p in basin i; q significant, in another basin of the list, a 26-neighbour of p inside
 *              the box) the PASS of a pair is whichever of D[p], D[q] has the smaller |D|; saddle is the pass with the greatest
 *              |D| (a signed float32 map value) and neighbour the smallest list index among the basins of the q's of the pairs
 *              that attain it.  Both are functions of the values alone.  Without such a pair -- exactly when the basin is its
 *              whole blob -- neighbour = -1 and saddle = 0.  Pairs with orphan voxels do not count.
 * basin: the box's voxels, [s][r][c] of the box, c fastest (uniqueNcrs[2] x uniqueNcrs[1] x uniqueNcrs[0]): the list index of the
 * voxel's basin, or -1 for insignificant and orphan voxels.
 * counters[4]: significant voxels, orphan voxels, pointer-doubling rounds run, bytes of device memory the job held.
 * An empty list succeeds: rows are untouched and basin, if given, is all -1.  PDBEDA_ERR_ARGUMENT before any launch: a NULL or
 * freed list.  PDBEDA_ERR_TIMEOUT on a context whose watchdog has expired.  The ascent is resolved by at most 31 doubling rounds
 * (enough for any path in a box of fewer than 2^31 voxels), enqueued in small batches with one wait per batch.  The rows are kept
 * with the list: a second call copies them without a launch (a call that asks for `basin` runs the job again: the volume is not
 * kept).  The result for either list of a fused job equals the single call's to the bit.  Synchronous; any output pointer may be
 * NULL; a failing call leaves the context usable. */
int pdbeda_peaklist_basins(pdbeda_peaklist *pl,
                           int64_t *n, double *sum, int64_t *s1 /* n_peaks x 3 */, double *sw1 /* n_peaks x 3 */,
                           float *saddle, int32_t *neighbour,
                           int32_t *basin   /* box voxels [us][ur][uc], c fastest; may be NULL */,
                           int64_t counters[4]);
/* Release a list (no reference counterpart; does not wait: the arena is recycled in stream order).  The handle is gone afterwards. */
int pdbeda_peaklist_free(pdbeda_peaklist *pl);

/* ---- regional sums ---------------------------------------------------------------- */
/* The voxel part of calculateRegionDiscrepancy / calculateRegionDensity
 * (densityAnalysis.py:1037-1068, 1160-1211): per group (atom or residue sphere-union,
 * deduplicated on raw crs): pos = sum of density > cutoff, neg = sum of density < -cutoff
 * (strict, cutils.pyx:245), n_region = |sphere union| with no density filter
 * (densityAnalysis.py:1198), valid = utils.testValidXyzList (cutils.pyx:273-313).
 * Any output pointer may be NULL.
 * A non-finite coordinate or radius: PDBEDA_ERR_ARGUMENT, the message names the atom, before anything is staged or launched; a
 * finite one beyond what the host may turn into grid indices leaves the sizing of the batch to the device (pdbeda_sphere_blobs). */
int pdbeda_region_sums(pdbeda_map *map, const double *xyz, const float *radii, int64_t n_atoms,
                       const int64_t *group_offsets, int64_t n_groups, float cutoff,
                       double *pos, double *neg, int64_t *n_region, uint8_t *valid);

/* ---- radial profiles -------------------------------------------------------------- */
/* The density around an atom by distance (no reference counterpart: the reference answers "what is inside ONE radius" --
 * getSphereCrsFromXyz, cutils.pyx:220-248 -- and the curve its radii were read from takes one call per candidate radius).
 * Per atom, ONE pass over the sphere box of `radius` -- [C - R - 1, C + R] per axis, C = xyz2crsCoord(atom),
 * R = xyz2crsCoord(origin + radius): the box of pdbeda_region_sums, which under-covers the sphere on skewed cells (Q4) and is
 * not widened here.  A voxel of the box is INSIDE when d <= (double)radius (float32 radius), d = sqrt((dx*dx + dy*dy) + dz*dz)
 * in unfused fp64 from crs2xyzCoord (ccp4.py:304-316) -- the sphere test of pdbeda_region_sums.  Its shell is
 *     k = min((int)floor(d / w), n_shells - 1),   w = (double)radius / (double)n_shells      (IEEE fp64 divisions)
 * so d == 0 lies in shell 0 and d == radius in the last shell.  Its density is utils.getPointDensityFromCrs (periodic wrap, 0
 * where nothing is stored).  Per atom and shell, [n_atoms][n_shells] row major:
 *   n        voxels of the shell, no density filter;
 *   sum      their density;
 *   n_sig, sum_sig   the same over the voxels that pass the strict filter of getSphereCrsFromXyz (cutils.pyx:245): density >
 *            cutoff for cutoff > 0, density < cutoff for cutoff < 0 (float32 cutoff); cutoff == 0: every voxel passes, so
 *            n_sig == n and sum_sig == sum;
 * and per atom: valid = utils.testValidXyzList of the sphere (0 when a voxel of it is not stored), as in pdbeda_region_sums.
 * A voxel's density enters a sum rounded once to the map's fixed-point quantum (<= 2^-38 max |rho| on maps of up to 2^22
 * voxels; the quantum of the blob sums, doubled per doubling of the largest box of the call beyond 2^22 voxels) and the sums are
 * folded as integers: bit-identical from run to run, within quantum / 2 per voxel of the exact sum; an empty shell is exactly 0.  Atoms do not see
 * each other: bonded atoms share voxels once radius exceeds half a bond length -- a profile is per atom, not a partition.
 * n_atoms == 0 succeeds and touches nothing.  PDBEDA_ERR_ARGUMENT before any launch: n_shells outside [1, PDBEDA_MAX_SHELLS],
 * a radius that is not finite or <= 0, a NaN cutoff, a non-finite coordinate, a box of 2^31 voxels or more, a coordinate or a
 * radius of 2^29 grid steps or more (the host makes the boxes, and casts nothing beyond that).  Synchronous. */
#define PDBEDA_MAX_SHELLS 64
int pdbeda_radial_profiles(pdbeda_map *map, const double *xyz, int64_t n_atoms, float radius, int32_t n_shells, float cutoff,
                           int64_t *n, double *sum, int64_t *n_sig, double *sum_sig, uint8_t *valid); /* any output may be NULL */

/* ---- nearest-atom map partition ----------------------------------------------------- */
/* Every voxel of the map to the atom nearest to it, counted ONCE (no reference counterpart: every per-atom number of the
 * reference, and pdbeda_region_sums / pdbeda_radial_profiles here, is a sphere around one atom, so a voxel beside a bond is
 * counted for a dozen atoms and the per-atom numbers add up to nothing).
 * Domain: the voxels of the non-repeating box header.uniqueNcrs -- the domain of createFullCrsList (ccp4.py:262-269, 452-461), of
 * the whole-map blob lists and of the peaks.  Nothing wraps and no voxel is counted twice.
 * Owner of voxel v: p = crs2xyzCoord(v) (ccp4.py:304-316); d2_a = (dx*dx + dy*dy) + dz*dz in unfused fp64 for every atom a; the
 * owner is the atom with the smallest d2, ties go to the LOWEST atom index (coincident atoms are allowed: the first owns).  The
 * owner counts only if sqrt(d2) <= (double)max_distance (IEEE sqrt, inclusive, float32 max_distance) -- the sphere test of
 * pdbeda_region_sums; if it does not, the voxel is UNOWNED (owner -1).  An atom far from the map simply owns nothing.
 * Per atom, [n_atoms] each:
 *   n                 voxels owned;
 *   sum               their density;
 *   n_pos / sum_pos   the owned voxels with density > cutoff;
 *   n_neg / sum_neg   the owned voxels with density < -cutoff      (strict, float32 cutoff >= 0: the filters of pdbeda_region_sums).
 * Over the unowned voxels: unowned_n = {n, n_pos, n_neg}, unowned_sum = {sum, sum_pos, sum_neg, sum_sq}; sum_sq is the fp64 sum of
 * the squares, folded in a fixed order (per workgroup, then over the workgroups in index order): n, sum and sum_sq give the mean
 * and the deviation of the map where there is no model.
 * owner: the box's voxels, [s][r][c] of the box, c fastest (uniqueNcrs[2] x uniqueNcrs[1] x uniqueNcrs[0]), the owner's index in
 * `xyz` or -1.
 * A NaN voxel (and an infinite one) is owned like any other and counted in n; it enters no density sum and neither filter.
 * A voxel's density enters a sum rounded once to the map's fixed-point quantum (the quantum of the blob sums: <= 2^-36 max |rho|)
 * and the sums are folded as integers: bit-identical from run to run, independent of the order of the atomics and -- apart from
 * the tie rule -- of the order of the atom list; within quantum / 2 per voxel of the exact sum; an atom that owns nothing gets
 * exact zeros.
 * n_atoms == 0 succeeds: everything is unowned.  PDBEDA_ERR_ARGUMENT before any launch: a max_distance that is not finite or
 * <= 0, a cutoff that is NaN or < 0, a non-finite coordinate, n_atoms >= 2^31.  Synchronous; a failing call leaves the context
 * usable. */
int pdbeda_map_partition(pdbeda_map *map, const double *xyz, int64_t n_atoms, float max_distance, float cutoff,
                         int64_t *n, double *sum, int64_t *n_pos, double *sum_pos, int64_t *n_neg, double *sum_neg, /* [n_atoms] each */
                         int64_t unowned_n[3], double unowned_sum[4],   /* n, n_pos, n_neg; sum, sum_pos, sum_neg, sum_sq */
                         int32_t *owner);                               /* box voxels, [s][r][c] of the box, c fastest; -1 = unowned */
                         /* any output may be NULL */

/* ---- the map between voxels: trilinear density, atom Q-scores ---------------------------- */
/* The density at arbitrary coordinates (no reference counterpart: getPointDensityFromXyz, ccp4.py:389-398, rounds to the nearest
 * voxel).  The fractional grid position f[3] of a point x, in crs order, is xyz2crsCoord (ccp4.py:288-302) without its round():
 * orthogonal cells q[i] = (x[i] - origin[i]) / gridLength[i]; otherwise q[i] = dot(deOrthoMat, x)[i] * xyzInterval[i] -
 * crsStart[map2xyz[i]] (the dot product as everywhere: fma(a2, v2, fma(a0, v0, a1 * v1))); f[j] = q[map2crs[j]].
 * b[j] = floor(f[j]), t[j] = f[j] - b[j]; the eight corners b + {0,1}^3 are read with utils.getPointDensityFromCrs (periodic wrap, 0
 * where nothing is stored), promoted to fp64, and folded with lerp(a, b, t) = a + t * (b - a) in unfused fp64 along c first, then r,
 * then s: t == 0 returns the base corner's value exactly whenever the other corner is finite, so the interpolant at a voxel centre IS
 * the voxel.  valid = 1 when all eight corners are stored (utils.testValidCrs), whatever their weights, else 0.  Non-finite voxels
 * propagate into the value.  n == 0 succeeds and touches nothing.  PDBEDA_ERR_ARGUMENT before any launch: a non-finite coordinate, a
 * coordinate whose grid position is 2^29 steps or more (the message names the point), n >= 2^31.  Synchronous; a failing call leaves
 * the context usable. */
int pdbeda_interp_density(pdbeda_map *map, const double *xyz, int64_t n, double *out, uint8_t *valid); /* either output may be NULL */

/* Per-atom Q-scores (Pintilie et al., Nature Methods 17, 2020): how well the map around an atom follows a reference Gaussian, read
 * on concentric spheres and only where the atom is the nearest one -- independent of the grid, unlike the voxel counts of
 * pdbeda_radial_profiles.  The host supplies the reference profile and the candidate directions (the device evaluates no exp, sin or
 * cos), and the directions are FIXED lattices, not random draws: values are reproducible, and are not MapQ's digit for digit.
 * Candidate levels: level l is the rows level_offsets[l] .. level_offsets[l + 1] of unit_pts ([..][3]); 1 <= n_levels <=
 * PDBEDA_QSCORE_MAX_LEVELS, every level 1 .. PDBEDA_QSCORE_MAX_LEVEL_POINTS rows, 1 <= min_points <= the size of level 0,
 * 2 <= n_shells <= PDBEDA_MAX_SHELLS.
 * Sample point of atom a, shell k (radius R_k = k * (double)step, float32 step), direction u: p[i] = a[i] + R_k * u[i], unfused fp64.
 * p is REJECTED when some atom b of xyz with an index other than a's has d2(p, b) < d2(p, a) (strict), d2 = (dx*dx + dy*dy) + dz*dz as
 * pdbeda_map_partition evaluates it; d2(p, a) is evaluated from p like the others (not taken as R_k^2), so atoms on a's coordinate tie
 * to the bit and reject nothing.  Nothing else rejects a point: acceptance does not depend on the map.
 * Shell 0 is the single point a, always kept.  Shell k >= 1 walks the levels in order, stops at the first level with at least
 * min_points accepted candidates and keeps ALL accepted candidates of that level; if no level reaches min_points it keeps the accepted
 * candidates of the last level, which may be none (MapQ's "add candidates until enough survive", with fixed lattices).
 * The value at a kept point is pdbeda_interp_density's.  Per scored atom: shell_n [n_shells] the kept points of a shell, shell_mean
 * their mean (exactly 0 for an empty shell), n_points the total, valid = 1 when every kept point was valid in pdbeda_interp_density's
 * sense, and q: the Pearson correlation over all kept points between the sampled value and ref[k] of the point's shell -- unchanged
 * under rho -> alpha * rho + beta with alpha > 0, so the reference needs no amplitude or offset -- clipped to [-1, 1].  q is NaN when
 * n_points < 2, when fewer than two shells kept a point, when the smallest and the largest sampled value are equal (an exact min /
 * max), when a sampled value is not finite, and when ref takes one value over the shells that kept a point (nothing to correlate with).
 * counters = {scored atoms (entries of `scored`) with more neighbours than the kernel stages at a time -- they take a slower path
 * with the same results --, the largest neighbour count seen}; a neighbour of a is an atom of xyz with another index within
 * 2 R_max (1 + 1e-6) of it, R_max = (n_shells - 1) * (double)step: farther atoms win no point.
 * No floating-point atomic and no sum across atoms: two calls agree to the bit, and so do calls whose xyz is permuted (scored re-mapped).
 * n_scored == 0 succeeds and touches nothing; with scored == NULL every atom is scored in order (n_scored is ignored) and n_all == 0
 * is the same.  PDBEDA_ERR_ARGUMENT before any launch: a limit above, a step that is not finite or <= 0, a non-finite ref, unit_pts or
 * coordinate, an index of scored outside [0, n_all) (repeats and any order are fine), n_all or n_scored >= 2^31, a scored atom whose
 * grid position, or an R_max whose extent along a grid axis, is 2^29 steps or more.  Synchronous; a failing call leaves the context
 * usable. */
#define PDBEDA_QSCORE_MAX_LEVELS 8
#define PDBEDA_QSCORE_MAX_LEVEL_POINTS 64
int pdbeda_atom_qscores(pdbeda_map *map,
                        const double *xyz, int64_t n_all,          /* every atom that competes for space: the symmetry atoms */
                        const int32_t *scored, int64_t n_scored,   /* indices into xyz of the atoms to score; NULL: all, in order */
                        float step, int32_t n_shells,              /* shell k has radius R_k = k * (double)step, k = 0 .. n_shells-1 */
                        const double *ref,                         /* [n_shells] reference profile, made by the host */
                        const double *unit_pts, const int32_t *level_offsets, int32_t n_levels, int32_t min_points,
                        double *q, int32_t *n_points,              /* [n_scored] */
                        int32_t *shell_n, double *shell_mean,      /* [n_scored][n_shells] */
                        uint8_t *valid, int64_t counters[2]);      /* any output may be NULL */

/* ---- from the model to a map: calculated density, map-model sums ------------------------- */
/* The density of a list of Gaussian atoms on the grid of a map (no reference counterpart: every other entry point reads observed
 * maps; ChimeraX calls this molmap).  Atom a is n_terms Gaussians, rho_a(d) = sum_j amp[a][j] * exp(-expo[a][j] * d^2), cut off at
 * radii[a].
 * Output and domain: *out is a NEW map owned by the library on the geometry of `like` -- ownership and lifetime are those of
 * pdbeda_map_combine's result (pdbeda_map_free).  Only the geometry of `like` is read, never its density.  The domain is ALL stored
 * voxels ncrs, not just the non-repeating box: the result is a complete map for every call that takes one.  Nothing wraps:
 * periodicity comes from the caller passing the symmetry images, as for pdbeda_map_partition.
 * A pair: p = crs2xyzCoord(v) (ccp4.py:304-316); d2 = (dx*dx + dy*dy) + dz*dz in unfused fp64, as pdbeda_map_partition evaluates
 * it; atom a contributes to voxel v iff sqrt(d2) <= (double)radii[a] (IEEE sqrt, inclusive) -- the sphere test of
 * pdbeda_region_sums.
 * A term: t = amp[a][j] * exp(-(expo[a][j] * d2)) with the device library's fp64 exp, one rounding for the product inside and one
 * for the product outside.  Amplitudes may be negative (omit and difference use); expo >= 0 (0: a constant inside the sphere).
 * Order independence: every term is rounded ONCE, half to even, to the quantum 2^-S and the terms of a voxel are added as 64-bit
 * integers; a thread owns its voxel, so there is no atomic at all.  S is the largest integer <= 40 with n_gridded * A_max * 2^S <=
 * 2^62, evaluated by the host in fp64: A_max = max over ALL atoms of sum_j |amp[a][j]| (added in index order), n_gridded = the atoms
 * inside the xyz bounding box of the stored voxels grown by slightly more than the largest radius (all others reach nothing);
 * S = 40 when A_max == 0 or no atom is gridded.  The voxel is float32((double)sum * 2^-S): one conversion, an exact scaling, one
 * rounding to nearest.  A voxel that no atom reaches is exactly +0.0f.  The value of a pair does not depend on the tile, the staging
 * run or the cell that meets it: two calls agree to the bit, and so do calls whose atom list is permuted.  Before the last
 * rounding a voxel is within (terms of the voxel) * 2^-S / 2 plus the error of exp of the exact sum.
 * counters = {S, the largest number of atoms a tile staged, the tiles that needed more than one staging run}.
 * n_atoms == 0 succeeds: an all-zero map.  PDBEDA_ERR_ARGUMENT before any launch: n_terms outside 1 .. PDBEDA_MODEL_MAX_TERMS, a
 * non-finite coordinate, amplitude or exponent, a negative exponent, a radius that is not finite or <= 0, n_atoms >= 2^31, a
 * radius whose extent along a grid axis is 2^29 steps or more, amplitudes whose n_gridded * A_max is not finite.  Synchronous; a
 * failing call leaves the context usable and *out untouched. */
#define PDBEDA_MODEL_MAX_TERMS 6
int pdbeda_model_density(pdbeda_map *like,
                         const double *xyz, int64_t n_atoms,      /* the atoms that contribute: the symmetry atoms for a crystal */
                         int32_t n_terms,                          /* Gaussians per atom, 1 .. PDBEDA_MODEL_MAX_TERMS */
                         const double *amp, const double *expo,    /* [n_atoms][n_terms] */
                         const float *radii,                       /* [n_atoms] cut-off distance of each atom */
                         pdbeda_map **out, int64_t counters[3]);   /* counters may be NULL */

/* The sums that correlate two maps of one grid shape: over the voxels of the non-repeating box header.uniqueNcrs (the domain of the
 * whole-map lists) where both values are finite and (double)b > (double)b_floor (strict; -INFINITY keeps every finite pair), n and
 * sums = {Sa, Sb, Saa, Sbb, Sab} in fp64, products unfused.  They give the correlation coefficient and the least-squares scale and
 * offset of a against b.  The fold has a fixed order -- a number of workgroups fixed by the box, per-workgroup partials, one block
 * over the partials in index order, as pdbeda_map_partition folds sum_sq --: the same maps give the same bits in every run.  An
 * empty selection gives n = 0 and sums of exactly 0.  PDBEDA_ERR_ARGUMENT: maps of different shapes or contexts, a NaN b_floor.
 * Synchronous; either output may be NULL. */
int pdbeda_map_pair_moments(pdbeda_map *a, pdbeda_map *b, float b_floor, int64_t *n, double sums[5]);  /* Sa, Sb, Saa, Sbb, Sab */

/* ---- from a map back to the atoms: the adjoint of the model density ------------------------- */
/* Per atom and Gaussian term the sums of a weight map against the atom's own Gaussian, against the Gaussian times the offset vector and
 * against the Gaussian times the squared distance (no reference counterpart).  With the weight map a residual obs - s * calc - o these are
 * the derivatives of the least-squares map-model target with respect to occupancy, position and B: what real-space refinement needs.
 * The pair set is EXACTLY pdbeda_model_density's: p = crs2xyzCoord(v); dx = p.x - x_a, likewise dy, dz; d2 = (dx*dx + dy*dy) + dz*dz in
 * unfused fp64; voxel v pairs with atom a iff sqrt(d2) <= (double)radii[a] (IEEE sqrt, inclusive).  Nothing wraps: the caller passes
 * the symmetry images, as for the model.
 * Domain: ALL stored voxels ncrs, the model's domain.  Under PDBEDA_MOMENTS_UNIQUE_BOX only the non-repeating box header.uniqueNcrs,
 * the domain of pdbeda_map_pair_moments: the sums are then derivatives of exactly the target that the correlation fits.
 * Terms: for atom a, term j, voxel v: e = exp(-(expo[a][j] * d2)) with the device library's fp64 exp, one rounding for the product
 * inside, as in the model; t0 = (double)w(v) * e; the five terms are t0, t0*dx, t0*dy, t0*dz, t0*d2, each product rounded once.
 * moments[a][j] = {M0, Mx, My, Mz, M2}, their sums over the atom's pairs.  Amplitudes do not enter: the sums are linear in them and
 * the host multiplies.  expo >= 0 (0: the plain moments of the weight inside the sphere).
 * Order independence: every term is rounded ONCE, half to even, to the quantum 2^-S and added as a 64-bit integer; an output is
 * (double)sum * 2^-S.  S = 61 - e with B < 2^e (the rule of every integer sum of the library; 40 where B is 0) for the bound B =
 * max|w| * max(1, r_max^2) * max(V_max, 2^22), evaluated by the host in fp64 in that order: max|w| the largest |w| over the STORED
 * map (one fixed-order reduction, cached with the map until pdbeda_map_invalidate), r_max = (double) of the largest radius, V_max
 * the voxels of the largest box (below).  Two calls agree to the bit; so do calls with the atoms permuted, rows re-mapped; and while S
 * is the same the result of an atom does not depend on which other atoms are in the call (only r_max and V_max tie them).
 * The box: the host covers every sphere with a box of crs indices -- half-width radius * |row k of the xyz -> crs matrix| along crs
 * axis k, which covers on any cell, skewed ones included, widened by 2^-30 of the magnitudes involved so that no rounding loses a
 * voxel -- and clips it to the domain.  The box only bounds the search: membership is the sphere test above.
 * n_voxels[a] = the pairs of atom a.  An atom that reaches no voxel of the domain has n_voxels = 0 and moments of exactly +0.0.
 * counters = {S, V_max, the atoms whose covering box the domain clipped (atoms wholly outside it included)}.
 * A weight map with non-finite voxels is refused with PDBEDA_ERR_ARGUMENT, as the labelling calls refuse it.  PDBEDA_ERR_ARGUMENT
 * before any launch: n_terms outside 1 .. PDBEDA_MODEL_MAX_TERMS, an unknown flag, n_atoms >= 2^31, a non-finite coordinate or
 * exponent, a negative exponent, a radius that is not finite or <= 0, a radius of 2^29 grid steps or more along a crs axis, a clipped
 * box of 2^31 voxels or more.  n_atoms == 0 succeeds and touches nothing.  Synchronous; a failing call leaves the context usable and
 * the outputs untouched. */
#define PDBEDA_MOMENTS_UNIQUE_BOX 1u
int pdbeda_atom_moments(pdbeda_map *weight,
                        const double *xyz, int64_t n_atoms,
                        int32_t n_terms,                    /* 1 .. PDBEDA_MODEL_MAX_TERMS */
                        const double *expo,                 /* [n_atoms][n_terms], >= 0 */
                        const float *radii,                 /* [n_atoms] */
                        uint32_t flags,
                        double *moments,                    /* [n_atoms][n_terms][5]: M0, Mx, My, Mz, M2 */
                        int32_t *n_voxels,                  /* [n_atoms] */
                        int64_t counters[3]);               /* any output may be NULL */

/* ---- what fits in a blob: rigid-fragment poses scored on a map ----------------------------- */
/* A small rigid fragment (a ligand, an ion, a side-chain conformer) tried under n_rot rotations at n_centres centres: every pose is
 * scored by the map read BETWEEN voxels at its atoms, and the best poses of every centre are ranked (no reference counterpart).
 * The fragment is frag_xyz [n_frag][3] relative to its pivot with weights frag_w [n_frag]; a rotation is a row-major 3x3 matrix made
 * by the host (the device evaluates no sin or cos).  Rotations are NOT checked for orthonormality: they are 3x3 matrices.
 * Position of atom a in pose (centre c, rotation R): p[i] = c[i] + dot(R[i], x_a), the dot product as everywhere, fma(R[i][2], x_a[2],
 * fma(R[i][0], x_a[0], R[i][1] * x_a[1])), then ONE unfused fp64 add.
 * Sample: v_a and valid_a are exactly pdbeda_interp_density's value and valid flag at p.  (A position that call would refuse -- not
 * finite, or 2^29 grid steps or more from the origin, which only a matrix that is no rotation can produce -- has v_a = NaN, valid_a = 0.)
 * Score: s = +0.0, then s = s + frag_w[a] * v_a for a = 0 .. n_frag-1: the product is rounded, then the sum, in unfused fp64.
 * A NaN score is stored as THE quiet NaN 0x7ff8000000000000, so that equal inputs give equal bytes on every path.
 * Low atoms: n_low = the atoms with v_a < (double)floor (a NaN on either side compares false).
 * A pose is REJECTED when n_low > max_low (a negative max_low rejects every pose), when its score is NaN, or when some valid_a == 0
 * unless PDBEDA_POSE_ALLOW_OUTSIDE is set.  Every other pose is kept.
 * Ranking: the kept poses of ONE centre, by score descending compared as numbers (-0.0 == +0.0), ties to the lower rotation index: a
 * strict total order.  best_rot [n_centres][top_k] the rotation indices in that order, -1 beyond the kept poses; best_score the scores,
 * +0.0 where the index is -1; best_low the poses' n_low, 0 where the index is -1; n_kept [n_centres] the kept poses of a centre.
 * The full table: all_score, all_low [n_centres][n_rot] and all_kept (1 / 0) of EVERY pose, rejected ones included (their score and
 * n_low are what the rules above give).
 * counters = {centres whose box was not staged in LDS and that read the map directly -- a slower path with the same results --, the
 * largest staged box in voxels, rejected poses in total}.  The box of a centre covers the sphere of radius max_a |x_a| =
 * max_a sqrt((x*x + y*y) + z*z) around it by pdbeda_atom_moments' box rule (any cell, skewed ones included), grown by two voxels on
 * every side (the interpolation's support and one of safety) and NOT clipped: it is filled through the wrap rule.  It is staged when
 * 4 bytes a voxel plus a stored bit a voxel (whole 64-bit words) fit 128 KiB.  No result depends on the box.
 * PDBEDA_POSE_GLOBAL_ONLY (an A/B and test switch): no box is staged; the same bytes out, counters[0] = n_centres, counters[1] = 0.
 * No floating-point atomic and no sum across poses: two calls agree to the bit; permuting the centres permutes the rows.
 * n_centres == 0 succeeds and touches nothing.  PDBEDA_ERR_ARGUMENT before any launch, in this order, the message naming the offender:
 * n_frag outside 1 .. PDBEDA_POSE_MAX_ATOMS, n_rot outside 1 .. PDBEDA_POSE_MAX_ROTATIONS, top_k outside 1 .. PDBEDA_POSE_MAX_TOP, an
 * unknown flag, n_centres < 0 or n_centres * n_rot >= 2^31, a non-finite fragment coordinate or weight, a non-finite rotation entry, a
 * non-finite centre, a fragment radius of 2^29 grid steps or more along a crs axis, a centre whose grid position is 2^29 steps or
 * more.  floor may be anything (NaN and -INFINITY count no atom as low).  Synchronous; a failing call leaves the context usable.
 * Large calls are cut into chunks of centres inside the call; the results do not depend on the cut. */
#define PDBEDA_POSE_MAX_ATOMS 256
#define PDBEDA_POSE_MAX_ROTATIONS 1048576
#define PDBEDA_POSE_MAX_TOP 64
#define PDBEDA_POSE_ALLOW_OUTSIDE 1u
#define PDBEDA_POSE_GLOBAL_ONLY 2u
int pdbeda_pose_scores(pdbeda_map *map,
                       const double *frag_xyz, const double *frag_w, int32_t n_frag,   /* [n_frag][3] relative to the pivot, [n_frag] */
                       const double *rot, int64_t n_rot,                                /* [n_rot][9], row-major 3x3 */
                       const double *centres, int64_t n_centres,                        /* [n_centres][3] */
                       float floor, int32_t max_low,                                    /* the low-atom rule */
                       int32_t top_k, uint32_t flags,
                       int32_t *best_rot, double *best_score, int32_t *best_low,        /* [n_centres][top_k] */
                       int32_t *n_kept,                                                 /* [n_centres] */
                       double *all_score, int32_t *all_low, uint8_t *all_kept,          /* [n_centres][n_rot] */
                       int64_t counters[3]);                                            /* any output may be NULL */

/* ---- from a map to a map through a neighbourhood: separable filters, local statistics ---- */
/* A separable filter of a resident map (no reference counterpart; every other map-to-map call is voxel-wise).
 * Output and domain: *out is a NEW map owned by the library on the geometry of `map` -- ownership and lifetime are those of
 * pdbeda_map_combine's result (pdbeda_map_free).  The domain is ALL stored voxels ncrs, as for pdbeda_model_density.
 * One axis with n = ncrs[axis] stored indices, I = crsInterval of that crs axis, radius R and 2R + 1 taps w:
 *   y[i] = sum_{k = -R .. R} w[k + R] * x~[i + k]
 * -- correlation form: w[0] multiplies the neighbour at i - R, taps need not be symmetric.  The sum is accumulated in fp64 from +0.0 in
 * ascending k, one rounding for the product and one for the sum (unfused).  x~[j] is the wrap rule of getPointDensityFromCrs
 * (cutils.pyx:125-145; what pdbeda_point_density and pdbeda_interp_density apply), on that axis alone: if j < 0 or j >= n then
 * j -= floor(j / I) * I; afterwards an index with n <= j < I is absent and contributes 0.0, an index in [I, n) is read as stored.  So a
 * full-cell map is filtered periodically however often R wraps round n, a cut-out sees zeros outside, a stored box larger than the cell
 * reads its own copies.
 * Three passes in the order c, r, s: the first reads the float32 map widened to fp64, the intermediates are fp64 and unrounded, the
 * result is rounded ONCE to float32, to nearest.  The passes commute mathematically; the bits are defined by this order.
 * PDBEDA_FILTER_RENORMALIZE: the fp64 result is divided by N = (W_c[c] * W_r[r]) * W_s[s] before the last rounding, W_axis[i] = sum_k
 * w[k + R] * present(i + k) in the same order and arithmetic (the host computes the three arrays inside the call); where N > 0 is false
 * the voxel is +0.0f.  A weighted mean then stays a mean at the faces of a cut-out.  Requires every tap >= 0.
 * A lane owns its output: no atomic, no reduction across lanes, two calls agree to the bit.  Values of the map that are not finite are
 * not screened; they propagate as IEEE arithmetic says (0 * inf is a NaN).
 * PDBEDA_ERR_ARGUMENT before any launch: a radius outside 0 .. PDBEDA_FILTER_MAX_RADIUS, a NULL or non-finite tap, a negative tap
 * under renormalisation, an unknown flag (also: an axis of 2^30 indices or more).  Synchronous; a failing call leaves the context usable
 * and *out untouched.  Scratch: two fp64 volumes of the map's size from a self-releasing device arena, returned at the end of the call. */
#define PDBEDA_FILTER_MAX_RADIUS 64
#define PDBEDA_FILTER_RENORMALIZE 1u
int pdbeda_map_filter(pdbeda_map *map,
                      const double *taps_c, int32_t radius_c,   /* 2 * radius + 1 weights for the column axis */
                      const double *taps_r, int32_t radius_r,
                      const double *taps_s, int32_t radius_s,
                      uint32_t flags, pdbeda_map **out);

/* Windowed moments of one map, or of two: local mean, standard deviation and z-score of a (and b), and the local correlation of a and b.
 * Taps as for pdbeda_map_filter, all >= 0.  F[.] is the three-pass filter above kept in fp64 WITHOUT the final rounding, applied to the
 * channels a, a a, and with b also b, b b, a b (the products formed in fp64 from the float32 values, hence exact); N as above.  Per
 * voxel, in unfused fp64:
 *   Ea = F[a] / N, Eaa = F[a a] / N;  t = Eaa - Ea * Ea;  va = (t > 0) ? t : 0;  sa = sqrt(va);
 *   d = (sa > std_floor) ? sa : std_floor;  z = (d > 0) ? ((double)a - Ea) / d : 0;      the same for b;
 *   cov = F[a b] / N - Ea * Eb;  cc = (va > 0 && vb > 0) ? clamp(cov / sqrt(va * vb), -1, 1) : 0.
 * Where N > 0 is false every output is 0: undefined cells are 0 and not NaN because the labelling calls refuse a map that holds a NaN
 * and z_a exists to be labelled.  Each requested output is a NEW float32 map (rounded once) with the ownership of pdbeda_map_filter's;
 * any output pointer may be NULL.  The maps are read once (the pass along c writes every channel).
 * PDBEDA_ERR_ARGUMENT in addition to pdbeda_map_filter's cases: a negative tap, a negative or NaN std_floor, b of another shape or
 * context, mean_b / std_b / cc requested without b.  Synchronous; a failing call leaves the context usable and every output pointer
 * untouched.  Scratch: fp64 volumes of the map's size from a self-releasing device arena, returned at the end of the call -- the
 * channels plus one: THREE for one map, SIX for a pair (the passes along r and s rotate the channels through the spare volume). */
int pdbeda_map_local_stats(pdbeda_map *a, pdbeda_map *b /* may be NULL */,
                           const double *taps_c, int32_t radius_c, const double *taps_r, int32_t radius_r,
                           const double *taps_s, int32_t radius_s, double std_floor,
                           pdbeda_map **mean_a, pdbeda_map **std_a, pdbeda_map **z_a,
                           pdbeda_map **mean_b, pdbeda_map **std_b, pdbeda_map **cc);   /* any may be NULL */

/* ---- from a REGION of a map to a map: the ordered spread of a mask ---- */
/* Dilation, erosion, opening, closing, bounded distance maps, soft edges and masking in one primitive (no reference counterpart): an integer
 * contract over a caller-made ORDERED table of offsets, as pdbeda_bloblist_nearest has.  Integer up to the last step:
 * Seeds: a stored voxel u is a seed iff (double)x[u] > (double)threshold, strict; under PDBEDA_SPREAD_BELOW iff (double)x[u] <
 * (double)threshold.  A NaN is never a seed; infinities compare as IEEE says.
 * Positions: an index j on an axis follows the wrap rule of pdbeda_map_filter, per axis: if j < 0 or j >= n then j -= floor(j / I) * I;
 * afterwards an index with n <= j < I is absent.  A position that is absent on any axis is no seed.  So a full-cell map spreads
 * periodically however often the reach wraps, a cut-out sees nothing outside, a stored box larger than its cell reads its own copies.
 * Rank: for every stored voxel v over ALL of ncrs, t(v) is the smallest t such that v + offsets[t] (n_offsets x 3: dc, dr, ds) is a seed,
 * and n_offsets if there is none.  The library gives the table no geometric meaning and does not check its order; duplicate offsets are
 * legal (the smallest t wins).
 * Value: *out is a NEW map on the geometry of `map` -- ownership and lifetime are those of pdbeda_map_combine's result (pdbeda_map_free).
 * Without `base` the voxel is values[t(v)] with its bits kept (values: n_offsets + 1 float32, the last for "no seed in reach"; NaN and
 * infinities are allowed).  With `base` it is float32((double)base[v] * (double)values[t(v)]): the product of two float32 is exact in
 * fp64, so this is ONE rounding; values that are not finite propagate.
 * counters (may be NULL): {seeds among the stored voxels, voxels with t < n_offsets, the path taken: 1 rows, 0 ordered walk}.  A table
 * whose every (dr, ds) row is a contiguous run of dc with ranks that fall to one minimum and rise behind it (every ball in ascending
 * distance is one) is searched row by row with two bit scans per row; any other table, and every table under PDBEDA_SPREAD_ROWS=0 in the
 * environment (read at every call), is walked in order.  The paths agree to the bit.
 * A lane owns its voxel: no atomic, no reduction of values across lanes; two calls agree to the bit.
 * PDBEDA_ERR_ARGUMENT before any launch: a NULL map, offsets, values or out; n_offsets outside 1 .. PDBEDA_SPREAD_MAX_OFFSETS; a component
 * beyond +-PDBEDA_SPREAD_MAX_REACH; a NaN threshold; an unknown flag; a base of another shape or context; an axis of 2^30 indices or more.
 * Synchronous; a failing call leaves the context usable and *out untouched.  Scratch: the table and two counts per tile, from a
 * self-releasing device arena. */
#define PDBEDA_SPREAD_MAX_OFFSETS 16384
#define PDBEDA_SPREAD_MAX_REACH 32        /* |dc|, |dr|, |ds| of every offset */
#define PDBEDA_SPREAD_BELOW 1u
int pdbeda_map_spread(pdbeda_map *map, float threshold, uint32_t flags,
                      const int32_t *offsets, int64_t n_offsets,   /* n x 3: dc, dr, ds; an ORDERED table */
                      const float *values,                          /* n_offsets + 1; the last: no seed in reach */
                      pdbeda_map *base /* may be NULL */,
                      pdbeda_map **out, int64_t counters[3] /* may be NULL */);

/* ---- from a map to a map on ANOTHER grid: resampling under coordinate operators ---- */
/* A resident map carried to the grid of `dst_geom` through one or more affine operators (no reference counterpart; every other call stays
 * on the grid the map came with): two entries on one grid, the density under symmetry mates, an average over NCS copies, a finer box.
 * Output and domain: *out is a NEW map on `dst_geom` -- ownership and lifetime are those of pdbeda_map_combine's result
 * (pdbeda_map_free); the domain is ALL stored voxels of `dst_geom`.  `ops` holds n_ops rows of 12 doubles [R | t] in orthogonal Angstrom, laid
 * out as for pdbeda_symmetry_atoms; an operator maps DESTINATION coordinates to SOURCE coordinates (a pull-back).
 * The library is built with -ffp-contract=off and the contract fixes bits.  For every destination voxel v:
 *  1. p = crs2xyz(dst, v) (DensityHeader.crs2xyzCoord's arithmetic, as pdbeda_crs2xyz).
 *  2. for operator k in index order: x[i] = ((R[i][0] * p[0] + R[i][1] * p[1]) + R[i][2] * p[2]) + t[i], unfused (pdbeda_symmetry_atoms' arithmetic).
 *  3. f = the fractional grid position of x in `src`, in crs order, as pdbeda_interp_density computes it.
 *  4. the snap: per axis r = rint(f[j]); if |f[j] - r| <= 2^-26 then f[j] = r.  2^-26 of a grid step is far above the rounding of steps 1 to 3
 *     at any realistic position and far below what a float32 result can show; a grid-compatible operator then lands ON voxels.
 *  5. the sample and its validity:
 *     order 0: the voxel at rint(f) (half to even) under the wrap rule of pdbeda_point_density; valid iff that voxel is stored.
 *     order 1: b = floor(f), t = f - b; on an axis with t == 0 only index b is used and the fold along it is skipped, otherwise b and b + 1;
 *              lerp(a, b, t) = a + t * (b - a) along c, then r, then s (pdbeda_interp_density's fold).
 *     order 3: taps b - 1 .. b + 2 with the Catmull-Rom weights
 *                w0 = ((-0.5 t + 1.0) t - 0.5) t,  w1 = ((1.5 t - 2.5) t) t + 1.0,  w2 = ((-1.5 t + 2.0) t + 0.5) t,  w3 = ((0.5 t - 0.5) t) t,
 *              per axis y = ((w0 v0 + w1 v1) + w2 v2) + w3 v3, products and sums unfused, along c, then r, then s; with t == 0 only b is used.
 *     orders 1 and 3 are valid iff every voxel the sample USES is stored (testValidCrs); a voxel of a skipped axis is neither read nor
 *     required -- which differs from the `valid` output of pdbeda_interp_density.  Voxels that are not finite propagate.
 *  6. by default the value is that of the FIRST valid operator and the count is 1 (0: no operator is valid); under PDBEDA_RESAMPLE_MEAN the
 *     value is the fp64 sum over the valid operators, from +0.0 in index order, divided by their count.
 *  7. count 0: the voxel is `fill`, its bits kept (a NaN is allowed), whatever `base` is.  Otherwise float32(value), or with `base`
 *     float32((double)base[v] + alpha * value) -- two fp64 roundings, as pdbeda_map_combine.  *coverage, if asked for, is a NEW map of
 *     float32(count).
 * A lane owns its voxel: no atomic on a value, no reduction across lanes, two calls agree to the bit.  Whether a tap comes from a box staged
 * in LDS or from a direct load changes no bit (PDBEDA_RESAMPLE_STAGE=0 in the environment turns staging off; A/B).
 * counters (may be NULL): voxels with count > 0, voxels with count 0, (tile, operator) pairs served from LDS, pairs served by direct loads.
 * PDBEDA_ERR_ARGUMENT before any launch: n_ops outside 1 .. PDBEDA_RESAMPLE_MAX_OPS; an order other than 0, 1, 3; an unknown flag; a
 * non-finite entry of `ops` or a non-finite alpha; a `base` of another shape or context than the destination; a destination axis below 1 or of
 * 2^30 indices or more; a source grid position of 2^29 steps or more -- evaluated on the host at the eight corners of the destination index
 * box grown by one voxel, under every operator (the map is affine: the extreme sits at a corner).  Synchronous, one launch, one wait; a
 * failing call leaves the context usable and every output pointer untouched. */
#define PDBEDA_RESAMPLE_MAX_OPS 192
#define PDBEDA_RESAMPLE_MEAN 1u        /* default: the first valid operator */
int pdbeda_map_resample(pdbeda_map *src, const pdbeda_geometry *dst_geom,
                        const double *ops /* n_ops x 12: rows of [R | t], orthogonal A, as pdbeda_symmetry_atoms */, int32_t n_ops,
                        int32_t order /* 0 nearest, 1 trilinear, 3 tricubic (Catmull-Rom) */, uint32_t flags, float fill,
                        pdbeda_map *base /* may be NULL; on dst_geom's shape */, double alpha,
                        pdbeda_map **out, pdbeda_map **coverage /* may be NULL */, int64_t counters[4] /* may be NULL */);

/* ---- reciprocal space: the 3-D Fourier transform of a resident map, and what works on a resident spectrum ---- */
/* The forward transform (no reference counterpart; every other map call works in real space).  *out is a NEW spectrum owned by the library
 * in a self-releasing device arena of the map's context (pdbeda_spectrum_free): the Hermitian half [ns][nr][nh] complex fp64, nh = nc / 2 + 1,
 * of numpy's rfftn convention -- unnormalised,
 *   F[k2][k1][k0] = sum_{s, r, c} x[s][r][c] * exp(-2 pi i (c k0 / nc + r k1 / nr + s k2 / ns)),   k0 = 0 .. nc / 2.
 * The domain is ALL stored voxels ncrs: the stored box is the period, whatever the cell is (for a crystal map transform the whole cell,
 * DensityMatrix.symmetryExpanded on ccp4.cellHeader; a cut-out is periodic in its own box).  The map is neither read for its geometry beyond
 * ncrs nor screened: values that are not finite propagate.
 * The bits are defined.  Lines are transformed along c, then r, then s.  A line of length n is the autosort (Stockham) mixed-radix transform of
 * pdb_eda_amd/csrc/pdbeda_fourier_line.h: the radices of n = 2^a 3^b 5^c 7^d are 4 (a / 2 times), 2 (if a is odd), 3, 5, 7 in this order, the
 * twiddles come from a host-made fp64 table w[k] = exp(-2 pi i k / n) with every component within 1 ulp and w[0], w[n/4], w[n/2], w[3n/4] exact,
 * every product and sum is plain unfused IEEE fp64 in the order that header states.  A row along c is run as a complex line whose imaginary
 * parts are zero (no half-length or two-rows-in-one trick), of which columns 0 .. nc / 2 are kept.  The same line gives the same bits wherever
 * it lies; a lane owns its outputs, there is no atomic, two calls agree to the bit, and tests/fourier_harness.cpp gives the same bits on a CPU.
 * PDBEDA_ERR_ARGUMENT before any launch: a NULL argument; an axis that is not plannable, i.e. not 2^a 3^b 5^c 7^d or above
 * PDBEDA_FFT_MAX_AXIS (the message names the axis and the next plannable length).  Synchronous; a failing call leaves the context usable and
 * *out untouched.  Scratch: none beyond the spectrum itself (the passes along r and s run in place) and, once per context and length, the table. */
#define PDBEDA_FFT_MAX_AXIS 1024
typedef struct pdbeda_spectrum pdbeda_spectrum;
int pdbeda_map_fft(pdbeda_map *map, pdbeda_spectrum **out);
/* The inverse transform: a NEW map on the geometry of `like`, with the ownership of pdbeda_map_combine's result; only the geometry of `like`
 * is read, and its ncrs must equal the shape the spectrum was made from.  Lines along s, then r, then c, with the conjugate twiddles; the
 * pass along c rebuilds the whole Hermitian line from the half (column k0 > nc / 2 is the conjugate of column nc - k0 OF THE SAME ROW of
 * the half-transformed data; the imaginary parts of column 0 and, for even nc, of column nc / 2 are ignored), and the voxel is
 * float32(re / (double)N), N = nc nr ns: one fp64 division, one rounding.  The spectrum is not changed.  PDBEDA_ERR_ARGUMENT: a NULL
 * argument, another context, another shape.  Synchronous; failing calls leave *out untouched.  Scratch: ONE spectrum-sized volume. */
int pdbeda_spectrum_inverse(pdbeda_spectrum *spec, pdbeda_map *like, pdbeda_map **out);
int pdbeda_spectrum_shape(pdbeda_spectrum *spec, int32_t ncrs[3]);                 /* the shape of the MAP the spectrum was made from */
int pdbeda_spectrum_download(pdbeda_spectrum *spec, double *out /* [ns][nr][nc/2+1][2] */);
int pdbeda_spectrum_free(pdbeda_spectrum *spec);
/* Single coefficients: out[i] = (re, im) of F at idx[i] = (k0, k1, k2), crs order.  Any integer index is reduced modulo its axis (floor
 * modulo); a coefficient of the missing half, k0 > nc / 2 after reduction, is the conjugate of F[(ns - k2) % ns][(nr - k1) % nr][nc - k0].
 * n == 0 succeeds.  PDBEDA_ERR_ARGUMENT: NULL arguments with n > 0, n < 0.  Synchronous. */
int pdbeda_spectrum_values(pdbeda_spectrum *spec, const int32_t *idx /* n x 3, crs order */, int64_t n, double *out /* n x 2 */);
/* The metric of the calls below is the CALLER's: six doubles {m00, m11, m22, m01, m02, m12} of the symmetric matrix M with s^2 = h^T M h
 * = 1 / d^2 for the frequency numbers h of the stored box as the period (ccp4.reciprocalMetric: M = (B^T B)^-1, the columns of B being
 * b_k = orthoMat[:, map2crs[k]] * ncrs[k] / crsInterval[k]).  For index j on an axis of n:  h = j if 2 j <= n, else j - n.  Then, in unfused
 * fp64 and in this order, every m multiplied by the EXACT integer product converted to fp64,
 *   s2 = ((m00 * (h0 h0) + m11 * (h1 h1)) + m22 * (h2 h2)) + 2 * ((m01 * (h0 h1) + m02 * (h0 h2)) + m12 * (h1 h2)).
 *
 * pdbeda_spectrum_scale multiplies every coefficient IN PLACE by a radial transfer function g(s2) given as a table over [0, s2_max]:
 *   t = s2 * ((n_table - 1) / s2_max)  (the quotient formed once, in fp64);  i = floor(t);
 *   g = table[i] + (t - i) * (table[i + 1] - table[i])  for 0 <= t < n_table - 1;  g = table[n_table - 1] at t == n_table - 1 exactly;
 *   g = beyond for t > n_table - 1;  g = table[0] where t >= 0 is false (a metric that is not positive definite).
 * Both components are multiplied by the real g: one rounding each.  A lane owns its coefficient.  PDBEDA_ERR_ARGUMENT before any launch: NULL
 * arguments, n_table outside 2 .. PDBEDA_SPECTRUM_MAX_TABLE, a non-finite metric, table entry or `beyond`, s2_max not finite or not > 0.
 * Synchronous; a failing call leaves the spectrum untouched. */
#define PDBEDA_SPECTRUM_MAX_TABLE 4096
int pdbeda_spectrum_scale(pdbeda_spectrum *spec, const double metric[6], const double *table, int32_t n_table, double s2_max, double beyond);
/* Sums over resolution shells of one spectrum, or of two of one shape.  A coefficient belongs to shell j iff edges[j] <= s2 < edges[j + 1]
 * (s2 as above); outside the edges it is dropped.  The sums run over the FULL spectrum, evaluated on the half: a coefficient of column 0 and,
 * for even nc, of column nc / 2 has weight w = 1, every other w = 2.  Per shell: count[j] = sum w (integers), and sums[j] = { sum w |A|^2,
 * sum w |B|^2, sum w Re(A conj B), sum w Im(A conj B) } with |A|^2 = Are Are + Aim Aim, Re = Are Bre + Aim Bim, Im = Aim Bre - Are Bim, unfused
 * fp64, each multiplied by w; the last three are exactly 0 when b is NULL.  (Over the full spectrum of two real maps Im(A conj B) of a
 * coefficient and of its mirror cancel; the fourth sum is that of the STORED half, columns 0 .. nc / 2, under these weights.)  The fold has a fixed order, as pdbeda_map_pair_moments folds: a
 * number of workgroups fixed by the shape, each over a contiguous run of coefficients in index order, per-workgroup per-shell partials, and a
 * fold of every shell's partials in an order fixed by that number (strided sums, then a binary tree); no floating-point atomic: the same
 * spectra with the same edges give the same bits in every run.
 * PDBEDA_ERR_ARGUMENT before any launch: NULL a, metric or edges; n_shells outside 1 .. PDBEDA_SPECTRUM_MAX_SHELLS; a non-finite metric or
 * edge; edges that do not strictly ascend; b of another shape or context.  Synchronous; either output may be NULL; a failing call leaves
 * the outputs untouched. */
#define PDBEDA_SPECTRUM_MAX_SHELLS 256
int pdbeda_spectrum_shells(pdbeda_spectrum *a, pdbeda_spectrum *b /* may be NULL */, const double metric[6],
                           const double *edges /* n_shells + 1, strictly ascending */, int32_t n_shells,
                           int64_t *count /* n_shells */, double *sums /* n_shells x 4 */);

/* ---- aggregateCloud ------------------------------------------------------------------ */
/* DensityAnalysis.aggregateCloud up to its statistics tail (densityAnalysis.py:571-731) as ONE call: the clouds of every
 * eligible atom (findAberrantBlobs, 603), the centroid-distance cut-off over all atoms (607), the best cloud and the pooled
 * clouds per atom (622-642), the bonded-atom overlap completeness (652-659), the residue clouds = clusters of a residue's
 * pooled clouds under testOverlap, merged (644-650, 661-690), the domain clouds = the same over everything pooled
 * (692-712) and the totals behind densityElectronRatio (714-731).  Voxel lists never leave the device.
 *
 * What tests/test_gpu_cloud.py pins beyond that: an atom whose alias is another atom gets that atom's clouds -- the sphere around
 * the shared coordinate with the ALIAS's radius -- measured from its own coordinate; when two pooled atoms of one residue share
 * a coordinate their clouds carry the later atom's electrons only, atoms of different residues each count.  A sphere may leave
 * the stored box: a voxel with a raw index below 0 or >= ncrs has the density of the voxel it wraps to by the cell's interval,
 * and density 0 (so it is in no cloud) where the cell is not stored there; centroids are those of the raw, unwrapped positions.  Among
 * equally distant clouds the first in list order is the best one; a residue without a pooled cloud has no row and leaves no gap
 * in the others' ordinals, which are the caller's.  n == 0, or no pooled cloud at all, succeeds with empty tables, zero totals,
 * every owner in state 0 and a NaN cut-off when no atom has a cloud.  PDBEDA_ERR_ARGUMENT for an alias, key, owner key or bonded
 * key out of range, for decreasing residue ordinals and for a non-finite coordinate or radius (the message names the atom; nothing
 * was staged or launched); a failing call leaves the context usable.  A finite coordinate or radius beyond what the host may turn
 * into grid indices leaves the sizing of both jobs to the device (pdbeda_sphere_blobs).
 *
 * The caller flattens what the reference reads from the structure, in the reference's iteration order
 * (residues with id[0] == ' ', their child atoms whose residue_atom name has an atom type and whose occupancy != 0): */
typedef struct pdbeda_cloud_atoms {
    int64_t n;                 /* eligible atoms */
    const double *xyz;         /* n x 3: atom.coord (float32 promoted exactly) */
    const float *radius;       /* n: radii[atom type]                                         densityAnalysis.py:603 */
    const double *weight;      /* n: electrons[residue_atom] * occupancy                      densityAnalysis.py:690, 718 */
    const int32_t *residue;    /* n: ordinal of the atom's residue, non-decreasing */
    const int32_t *alias;      /* n: LAST eligible atom with the same coordinate (allAtomClouds is keyed by coordinate, 604) */
    const int32_t *key;        /* n: id of (residue, residue_atom name); atomCloudIndeces is keyed by the name (640) */
    int64_t n_keys;
    const int64_t *bonded_off; /* n_keys + 1: CSR over keys ... */
    const int32_t *bonded;     /* ... of the keys of bondedAtoms[name] that exist in the same residue      (656) */
    int64_t n_owners;          /* child atoms (ANY occupancy) of ATOM residues whose name has a key, in iteration order (653-655) */
    const int32_t *owner_key;
} pdbeda_cloud_atoms;

typedef struct pdbeda_cloud pdbeda_cloud; /* the result tables (host memory owned by the library) */

int pdbeda_aggregate_cloud(pdbeda_map *map, const pdbeda_cloud_atoms *atoms, float density_cutoff, double min_cloud_electrons,
                           pdbeda_cloud **out);
/* counts[4] = atom rows, residue-cloud rows, domain-cloud rows, owners;
 * totals[4] = numVoxels, totalElectrons, totalDensity (718-721, over ALL domain clouds), centroidDistanceCutoff (607). */
int pdbeda_cloud_counts(pdbeda_cloud *c, int64_t counts[4], double totals[4]);
/* One row per atom that has a best cloud, in iteration order (atomList, 642): index into the eligible atoms, the best
 * cloud's totalDensity, voxel count, centroid (x3) and |atom - centroid|.  Any pointer may be NULL. */
int pdbeda_cloud_atom_rows(pdbeda_cloud *c, int32_t *atom, double *total_density, int64_t *n_voxels, double *centroid, double *distance);
/* Residue clouds with >= min_cloud_electrons, in the reference's emission order (residue by residue; inside a residue by
 * lowest pooled-cloud index -- the reference's own order there follows CPython's set iteration): residue ordinal,
 * totalDensity, voxels, electrons, centroid (x3). */
int pdbeda_cloud_residue_rows(pdbeda_cloud *c, int32_t *residue, double *total_density, int64_t *n_voxels, double *electrons, double *centroid);
/* Domain clouds with >= min_cloud_electrons (unsorted: the caller sorts by ratio, 730): a representative residue ordinal
 * (the reference's is set-order dependent), totalDensity, voxels, electrons, centroid (x3). */
int pdbeda_cloud_domain_rows(pdbeda_cloud *c, int32_t *residue, double *total_density, int64_t *n_voxels, double *electrons, double *centroid);
/* Per owner: 0 = its name has no pooled cloud, 1 = every bonded partner's clouds touch its own, 2 = some do not (656-659). */
int pdbeda_cloud_owner_states(pdbeda_cloud *c, uint8_t *state);
int pdbeda_cloud_free(pdbeda_cloud *c);

/* ---- voxel-set adjacency ---------------------------------------------------------- */
/* utils.testOverlap (cutils.pyx:8-25) batched: pair p tests set a_idx[p] against set
 * b_idx[p]; sets are slices [set_offsets[i], set_offsets[i+1]) of crs. */
int pdbeda_test_overlap(pdbeda_ctx *ctx, const int32_t *crs, const int64_t *set_offsets, int64_t n_sets,
                        const int32_t *a_idx, const int32_t *b_idx, int64_t n_pairs, uint8_t *out);

/* ---- symmetry atoms --------------------------------------------------------------- */
/* utils.createSymmetryAtoms (cutils.pyx:73-103): x' = R x + t + orthoMat (i,j,k) for
 * (i,j,k) in {-1,0,1}^3 x ops, kept when inside bbox +- 5 A; the identity keeps all.
 * Outputs in the reference's order; returns the count through n_out (capacity cap). */
int pdbeda_symmetry_atoms(pdbeda_ctx *ctx, const double *xyz, int64_t n_atoms, const double *rot /* n_ops x 12 */,
                          int32_t n_ops, const double ortho[9], const double bbox_lo[3], const double bbox_hi[3],
                          int32_t *atom_index, int32_t *symmetry /* x4 */, double *out_xyz, int64_t cap, int64_t *n_out);
/* calculateAtomSpecificBlobStatistics inner step (densityAnalysis.py:932-935): for every
 * centroid the nearest atom (first index on ties, fp64 Euclidean as scipy cdist). */
int pdbeda_nearest_atom(pdbeda_ctx *ctx, const double *centroids, int64_t n_centroids, const double *atom_xyz,
                        int64_t n_atoms, int64_t *index, double *distance);

/* ---- crystal contacts --------------------------------------------------------------- */
/* crystalContacts.findCoordContacts (crystalContacts.py:87-101): for every query point
 * q_xyz[i] the minimum fp64 distance to the points p_xyz, reported as (i, distance) in
 * ascending i when <= cutoff (boundary included).  Returns the row count through n_out;
 * PDBEDA_ERR_CAPACITY when it exceeds cap (n_q always suffices).  cutoff must be finite
 * and > 0, every coordinate finite.  One wait. */
int pdbeda_coord_contacts(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, const double *p_xyz, int64_t n_p,
                          double cutoff, int64_t *out_index, double *out_distance, int64_t cap, int64_t *n_out);
/* crystalContacts.main + simulateCrystalNeighborCoordinates (crystalContacts.py:37-84,
 * 104-142) without pymol.  Image c of the candidate list cand[4c..4c+3] = (op, n0, n1, n2)
 * maps x to R_op x + t_op + ortho (n0, n1, n2) (rot: n_ops x 12 as in
 * pdbeda_symmetry_atoms; the same arithmetic).  (op 0, n = 0) is the asymmetric unit and
 * is refused.  Image c is kept (kept_out[c] = 1, optional) when some image of a poly_xyz
 * point lies within cutoff of some poly_xyz point; the query rows are then those of
 * pdbeda_coord_contacts against every point of every kept image.  Two waits. */
int pdbeda_crystal_contacts(pdbeda_ctx *ctx, const double *q_xyz, int64_t n_q, const double *poly_xyz, int64_t n_poly,
                            const double *rot /* n_ops x 12 */, int32_t n_ops, const double ortho[9],
                            const int32_t *cand /* n_cand x 4 */, int64_t n_cand, double cutoff, uint8_t *kept_out,
                            int64_t *out_index, double *out_distance, int64_t cap, int64_t *n_out);
/* The neighbour list of simulateCrystalNeighborCoordinates (crystalContacts.py:104-142):
 * the points of the listed images in (image, point) order, n_cand x n_poly x 3 doubles. */
int pdbeda_image_coords(pdbeda_ctx *ctx, const double *poly_xyz, int64_t n_poly, const double *rot /* n_ops x 12 */,
                        int32_t n_ops, const double ortho[9], const int32_t *cand /* n_cand x 4 */, int64_t n_cand,
                        double *out_xyz);

#ifdef __cplusplus
}
#endif
#endif /* PDBEDA_H */
