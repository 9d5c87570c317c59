"""The seeded inputs of tests/test_voxelsets_host.py and tests/test_gpu_voxelsets.py: explicit voxel lists for pdbeda_list_blobs,
voxel sets for pdbeda_test_overlap, atoms and centroids for pdbeda_nearest_atom, operators for pdbeda_symmetry_atoms and points
for the point helpers.  Importable without a GPU: nothing here touches the native library.  The worlds are the two maps of
tests/batch_limit_cases.py."""
import functools
import io
import types

import numpy as np

import batch_limit_cases
import profiles_checker

WORLDS = batch_limit_cases.WORLDS

# The two staging limits of the host library (pdb_eda_amd/csrc/pdbeda_hip.hip) that the sizes below are chosen around:
STAGED_ROW = 256 << 10          # h2d_row(): an input row goes through the pinned block only up to max_span = 256u << 10 bytes
PINNED_BLOCK = 4 << 20          # pdbeda_ctx_create: hipHostMalloc(&ctx->pinned, 4 << 20): what pinned_in / pinned_out hand out per call
PINNED_LINE = 64                # pinned_span(): a take occupies whole 64-byte lines

LIST_ROW = 12                   # bytes of a voxel of pdbeda_list_blobs (3 x int32)
SMALL_GROUPS = 3000
WIDTHS = (63, 64, 65, 130)


def pinned_span(n_bytes):
    return (n_bytes + PINNED_LINE - 1) // PINNED_LINE * PINNED_LINE


@functools.lru_cache(maxsize=None)
def world(name):
    """header, grid, file bytes and the +-1.5 sigma cutoff of a world, made with the host-side parser alone."""
    from pdb_eda_amd import ccp4, synthetic
    spec, grid = batch_limit_cases.spec_and_grid(name)
    raw = synthetic.ccp4_bytes(spec, grid)
    header, _ = ccp4.read_grid(io.BytesIO(raw))
    g64 = grid.astype(np.float64)
    cut = float(np.float32(g64.mean() + 1.5 * g64.std()))
    return types.SimpleNamespace(name=name, spec=spec, grid=grid, raw=raw, header=header, cut=cut, ncrs=[int(v) for v in header.ncrs],
                                 interval=[int(v) for v in header.crsInterval], top=float(np.abs(grid).max()))


def density(w, crs):
    """utils.getPointDensityFromCrs of raw crs rows (periodic wrap, 0 where nothing is stored), in numpy."""
    return profiles_checker.point_density(w.header, w.grid, np.asarray(crs, dtype=np.int64).reshape(-1, 3))[0]


def box(lo, dims):
    lo = [int(v) for v in lo]
    return profiles_checker.box_voxels(lo, [lo[k] + int(dims[k]) - 1 for k in range(3)])


def signed(w, vox, sign):
    """The voxels of vox above +cut (sign > 0) or below -cut."""
    rho = density(w, vox)
    return vox[rho > w.cut] if sign > 0 else vox[rho < -w.cut]


def random_lo(w, rng, dims):
    """A box origin such that the box stays within 6 voxels of the stored grid, and may reach that far on either side."""
    return [int(rng.integers(-6, w.ncrs[k] + 6 - int(dims[k]) + 1)) for k in range(3)]


EMPTY = np.zeros((0, 3), dtype=np.int64)


def _small_groups(w, rng):
    """(a): 0 to 9 one-sign voxels of a random box of 4 to 9 voxels a side; a group drawn with 0 voxels, and the runs set below, are empty."""
    out = []
    for g in range(SMALL_GROUPS):
        k = int(rng.integers(0, 10))
        keep = EMPTY
        for _ in range(50 if k else 0):
            dims = rng.integers(4, 10, size=3)
            keep = signed(w, box(random_lo(w, rng, dims), dims), 1 if rng.integers(0, 2) else -1)
            if len(keep):
                break
        if len(keep) > k:
            keep = keep[rng.choice(len(keep), k, replace=False)]
        out.append(keep[rng.permutation(len(keep))])
    for a, b in ((300, 305), (1700, 1703), (2990, 2993)):          # runs of consecutive empty groups
        for g in range(a, b):
            out[g] = EMPTY
    return out


def _width_group(w, rng, width):
    """(c): the voxels above the cutoff of a box width x 8 x 8 whose first and last c plane both hold one: a bounding box exactly `width` wide."""
    for _ in range(1000):
        dims = (width, 8, 8)
        lo = [int(rng.integers(-6, 6)), int(rng.integers(-6, w.ncrs[1] - 2)), int(rng.integers(-6, w.ncrs[2] - 2))]
        keep = signed(w, box(lo, dims), 1)
        if len(keep) and keep[:, 0].min() == lo[0] and keep[:, 0].max() == lo[0] + width - 1:
            return keep[rng.permutation(len(keep))]
    raise AssertionError("no box of width %d" % width)


def _dense_group(w, rng, dims, least):
    for _ in range(1000):
        keep = signed(w, box(random_lo(w, rng, dims), dims), 1 if rng.integers(0, 2) else -1)
        if len(keep) >= least:
            return keep
    raise AssertionError("no group of %d voxels" % least)


@functools.lru_cache(maxsize=None)
def list_groups(name):
    """The voxel list of a world: .crs (n x 3 int32, raw), .off (group_offsets, int64), .kind (per group: "a", "b", "c63" .. "c130",
    "d", "e", "f", "g", "z" or "-" for the forced empty first and last group), .groups (the per-group arrays).
    Order: an empty group, 1000 of (a), (e), (b), 1000 of (a), the four of (c), 20 of (d), (e) again, three of (f), the (g)s, 1000 of
    (a), an empty group."""
    w = world(name)
    rng = np.random.default_rng(8800 + WORLDS.index(name))
    small = _small_groups(w, rng)
    # (b) every voxel above the cutoff of a box of 136 x 128 x 100 that reaches past the stored grid on all sides (periodic images included)
    big = signed(w, box((-44, -40, -30), (136, 128, 100)), 1)
    big = big[rng.permutation(len(big))]
    widths = [_width_group(w, rng, width) for width in WIDTHS]
    dups = []
    for _ in range(20):          # (d) a third of the voxels twice, shuffled
        keep = _dense_group(w, rng, (8, 8, 8), 6)
        rows = np.concatenate([np.arange(len(keep)), rng.choice(len(keep), len(keep) // 3, replace=False)])
        dups.append(keep[rng.permutation(rows)])
    twin = _dense_group(w, rng, (10, 10, 10), 20)          # (e) one voxel set, given to two groups in two orders
    twins = [twin[rng.permutation(len(twin))], twin[rng.permutation(len(twin))]]
    images = []
    flat = np.argsort(-np.abs(w.grid).reshape(-1))
    for k in range(3):          # (f) a stored voxel and its periodic image one interval along crs axis k
        s, r, c = np.unravel_index(int(flat[k]), w.grid.shape)
        v = np.array([c, r, s], dtype=np.int64)
        shift = np.zeros(3, dtype=np.int64)
        shift[k] = w.interval[k]
        images.append(np.stack([v, v + shift if k != 1 else v - shift]))
    free = [box(random_lo(w, rng, (4, 3, 3)), (4, 3, 3)) for _ in range(8)]          # (g) every voxel of a small box
    zero = []
    if w.interval[1] > w.ncrs[1]:          # skew: rows ncrs[1] .. interval[1] - 1 of the cell are not stored
        free += [box((int(rng.integers(-6, w.ncrs[0])), r0, int(rng.integers(-6, w.ncrs[2]))), (4, 3, 3)) for r0 in (w.ncrs[1] - 2, w.ncrs[1] - 1, -3, -2)]
        zero = [box((5, w.ncrs[1] + 1, 7), (3, w.interval[1] - w.ncrs[1] - 2, 2))]          # nothing but unstored voxels: total density exactly 0
    groups = ([EMPTY] + small[:1000] + [twins[0], big] + small[1000:2000] + widths + dups + [twins[1]] + images + free + zero + small[2000:] + [EMPTY])
    kind = (["-"] + ["a"] * 1000 + ["e", "b"] + ["a"] * 1000 + ["c%d" % x for x in WIDTHS] + ["d"] * 20 + ["e"] + ["f"] * 3 + ["g"] * len(free) +
            ["z"] * len(zero) + ["a"] * 1000 + ["-"])
    assert len(groups) == len(kind)
    return _pack(groups, kind, np.arange(len(groups)))


def _pack(groups, kind, source):
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    crs = np.ascontiguousarray(np.concatenate(groups).astype(np.int32))
    return types.SimpleNamespace(crs=crs, off=off, kind=list(kind), groups=[np.asarray(g, dtype=np.int32) for g in groups], source=np.asarray(source))


def list_variants(name):
    """{"full": the list; "head": its first 900 groups (a few thousand voxels: below STAGED_ROW / LIST_ROW = 21 845, so the voxels
    travel as a staged row); "middle": every group but (b), three times over (more than 21 845 voxels but fewer than the 65 536 at which
    the per-voxel group ids, 4 bytes each, stop being staged too)}.  .source[g] is the group's index in the full list."""
    full = list_groups(name)
    head = _pack(full.groups[:900], full.kind[:900], np.arange(900))
    rest = [g for g in range(len(full.groups)) if full.kind[g] != "b"]
    middle = _pack([full.groups[g] for g in rest] * 3, [full.kind[g] for g in rest] * 3, np.array(rest * 3))
    return {"full": full, "head": head, "middle": middle}


def fold_sets(name):
    """Disconnected voxel sets for DeviceMap.list_stats (DensityBlob.fromCrsList / merge): (label, part A, part B), the parts disjoint
    and not adjacent.  One-sign pairs from the middle of the stored box; in skew also a one-sign blob with the all-unstored box of
    list_groups, a component whose total density is exactly 0."""
    w = world(name)
    rng = np.random.default_rng(8900 + WORLDS.index(name))
    out = []
    while len(out) < 3:
        a = signed(w, box((6, 6, 6), (5, 5, 5)), 1)
        lo = [int(rng.integers(14, w.ncrs[k] - 8)) for k in range(3)]
        b = signed(w, box(lo, (6, 6, 6)), 1 if len(out) != 1 else -1)
        if len(a) and len(b):
            out.append(("pair%d" % len(out), a, b))
    full = list_groups(name)
    for g, k in enumerate(full.kind):
        if k == "z":
            out.append(("zero", out[0][1], full.groups[g].astype(np.int64)))
    return out


# ---- pdbeda_test_overlap ---------------------------------------------------------------------------------------------------------
def overlap_sets():
    """.crs / .off: the sets; .pairs: (a_idx, b_idx, what) rows.  A base set of size n is n - 1 random voxels of a region of its own (all
    regions at least 50 voxels apart) and a LAST voxel far from everything; a partner set built on it touches, or misses by two, through
    its own last voxel alone: the only deciding voxel pair is the last (a, b) of the |A| x |B| walk."""
    rng = np.random.default_rng(8700)
    sets, pairs = [], []
    region = [0]

    def scatter(n):
        region[0] += 1
        lo = np.array([-400 + 90 * region[0], -37, -11])
        cells = rng.choice(30 * 30 * 30, n, replace=False)
        return lo + np.stack([cells % 30, (cells // 30) % 30, cells // 900], axis=1)

    def lonely():
        region[0] += 1
        return np.array([-400 + 90 * region[0], 300 + 7 * region[0], -200])

    def add(vox):
        sets.append(np.asarray(vox, dtype=np.int64).reshape(-1, 3))
        return len(sets) - 1

    empty = add(EMPTY)
    sizes = (1, 255, 256, 257, 1500)
    base, last = {}, {}
    for n in sizes:
        last[n] = lonely()
        base[n] = add(np.concatenate([scatter(n - 1), last[n][None]]))
    for na, nb, step in ((1, 1, (1, 1, 1)), (255, 257, (1, -1, 0)), (256, 256, (-1, 0, 1)), (257, 255, (0, 1, -1)), (1500, 1500, (1, 1, -1)), (1500, 1, (-1, -1, -1)),
                         (1, 1500, (0, 0, 1))):
        partner = add(np.concatenate([scatter(nb - 1), (last[na] + np.array(step))[None]]))
        pairs.append((base[na], partner, "touch %d x %d at the last pair" % (na, nb)))
        pairs.append((partner, base[na], "touch %d x %d at the last pair" % (nb, na)))
    for na, nb, step in ((255, 256, (2, 0, 0)), (256, 257, (0, -2, 0)), (257, 1500, (0, 0, 2)), (1, 1, (-2, 0, 0))):
        partner = add(np.concatenate([scatter(nb - 1), (last[na] + np.array(step))[None]]))
        pairs.append((base[na], partner, "miss by 2 on one axis, %d x %d" % (na, nb)))
    for n in sizes:
        pairs.append((base[n], base[n], "a set of %d against itself" % n))
        pairs.append((empty, base[n], "the empty set against %d" % n))
        pairs.append((base[n], empty, "%d against the empty set" % n))
    pairs.append((empty, empty, "the empty set against itself"))
    pairs.append((base[255], base[1500], "sets apart, the whole walk"))
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return types.SimpleNamespace(crs=np.ascontiguousarray(np.concatenate(sets).astype(np.int32)), off=off, sets=sets, pairs=pairs, sizes=sizes)


# ---- pdbeda_nearest_atom -----------------------------------------------------------------------------------------------------------
ATOM_COUNTS = (1, 255, 256, 257, 1000, 12000)          # 12 000 x 24 bytes = 288 000 > STAGED_ROW


def _grid_points(rng, n, lo, hi):
    """n distinct points on the 1/8 A lattice (every coordinate, sum and half-difference below is exact in fp64)."""
    pts = np.unique(rng.integers(int(lo * 8), int(hi * 8), size=(2 * n + 16, 3)), axis=0)
    pts = pts[rng.permutation(len(pts))][:n]
    assert len(pts) == n
    return pts.astype(np.float64) / 8.0


def nearest_case(n_atoms, n_random=40):
    """.atoms, .centroids, .ties = [(centroid row, lower atom index, higher atom index, what)].
    Duplicates: atom j is a copy of atom i for j - i = 1, 256 and 256 k + 3 (as far as n_atoms allows); a centroid ON atom i (distance 0) and one
    0.01 A beside it tie between i and j.  Mirror pairs: two atoms of a pair differ in x only, by 2 A, and sit 100 A and more from everything
    else; a centroid with the pair's middle x is equidistant from both (dx = +1 and -1 exactly)."""
    rng = np.random.default_rng(8600 + n_atoms)
    atoms = _grid_points(rng, n_atoms, -20.0, 60.0)
    ties = []
    cen = [rng.uniform(-25.0, 65.0, size=(n_random, 3))]
    rows = [n_random]

    def centroid(p, lo, hi, what):
        cen.append(np.asarray(p, dtype=np.float64)[None])
        ties.append((rows[0], lo, hi, what))
        rows[0] += 1

    gaps = [1] * (n_atoms >= 2) + [256] * (n_atoms >= 257) + [256 * (40 if n_atoms >= 12000 else 2) + 3] * (n_atoms >= 1000)
    for gap, i in zip(gaps, (2, 0, 4)):          # (atoms 2 = 3, 0 = 256, 4 = 4 + gap)
        j = i + gap
        atoms[j] = atoms[i]
        centroid(atoms[i], i, j, "on a duplicated atom, indices %d apart" % gap)
        centroid(atoms[i] + np.array([0.01, 0.0, -0.0078125]), i, j, "beside a duplicated atom, indices %d apart" % gap)
    if n_atoms >= 255:
        for k, gap in enumerate(gaps + [7]):
            i = 100 + 11 * k
            j = i + gap
            if j >= n_atoms:
                continue
            mid = np.array([300.0 + 150.0 * k, -140.0, 90.0])
            atoms[i] = mid + np.array([1.0, 0.0, 0.0])
            atoms[j] = mid - np.array([1.0, 0.0, 0.0])
            centroid(mid + np.array([0.0, 0.5, -0.25]), i, j, "mirrored in x, indices %d apart" % gap)
            centroid(mid, i, j, "the middle of a mirror pair, indices %d apart" % gap)
    return types.SimpleNamespace(atoms=np.ascontiguousarray(atoms), centroids=np.ascontiguousarray(np.concatenate(cen)), ties=ties)


def nearest_cases():
    return [nearest_case(n) for n in ATOM_COUNTS]


CENTROID_ROW = 16          # bytes of results per centroid: an int64 index and a double distance, one pinned_out() each


def nearest_batch_sizes():
    """Centroid counts around the two result arrays of pdbeda_nearest_atom, 8 bytes a centroid each, against 300 atoms.  Such a batch's inputs
    (24 bytes a centroid, far more than STAGED_ROW) are copied from the caller's memory, so the results have the 4 MiB block to themselves:
    index and distance both fit up to PINNED_BLOCK / CENTROID_ROW = 262 144 centroids; from 262 145 the index (taken first) fits alone, up to
    PINNED_BLOCK / 8 = 524 288; from 524 289 neither does.  -> (both, index only, index only at its edge, neither)."""
    both = PINNED_BLOCK // CENTROID_ROW
    index_only = PINNED_BLOCK // (CENTROID_ROW // 2)
    assert 2 * pinned_span(8 * both) == PINNED_BLOCK and 24 * both > STAGED_ROW
    return both, both + 1, index_only, index_only + 1


# ---- pdbeda_symmetry_atoms ---------------------------------------------------------------------------------------------------------
def _operators(n_ops):
    """n_ops x 12 (rows of [R | t]): the identity, then a two-fold screw, a three-fold about (1, 1, 1) with a translation, and a mirror-glide."""
    ops = [np.hstack([np.eye(3), np.zeros((3, 1))]),
           np.hstack([np.diag([-1.0, -1.0, 1.0]), np.array([[15.0], [0.0], [16.5]])]),
           np.hstack([np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[-3.25], [7.5], [11.0]])]),
           np.hstack([np.diag([1.0, -1.0, 1.0]), np.array([[4.0], [13.5], [-8.25]])])]
    return np.ascontiguousarray(np.stack(ops[:n_ops]).reshape(n_ops, 12))


SKEWED_ORTHO = np.array([[30.0, -8.5, 3.25], [0.0, 27.0, -5.5], [0.0, 0.0, 33.0]])


def symmetry_atoms_xyz(n):
    """float32 coordinates promoted to fp64, as the reference's atoms are; the first n of one seeded cloud of 2 000."""
    rng = np.random.default_rng(8500)
    return np.ascontiguousarray(rng.uniform([-4.0, 2.0, -9.0], [24.0, 25.0, 21.0], size=(2000, 3)).astype(np.float32).astype(np.float64)[:n])


def symmetry_cases():
    """(label, xyz, rot, ortho, bbox_lo, bbox_hi).  27 n_ops n_atoms = 999, 5 454 and 35 964 are multiples of neither 64 nor 256 (k_symmetry_keep
    writes a word per 64 candidates, 256 to a block); "tight": a box of 3 A in the cloud's middle, so most images fall outside box + 5 A;
    "huge": every one of the 27 x 4 x 2 000 = 216 000 images survives -- its list of survivors (8 bytes each) still fits the 4 MiB pinned
    block, its coordinates (24 bytes each, 5.2 MB) do not."""
    out = []
    for label, n_ops, n_atoms in (("one", 1, 37), ("two", 2, 101), ("four", 4, 333)):
        xyz = symmetry_atoms_xyz(n_atoms)
        out.append((label, xyz, _operators(n_ops), SKEWED_ORTHO, xyz.min(axis=0), xyz.max(axis=0)))
    xyz = symmetry_atoms_xyz(333)
    out.append(("tight", xyz, _operators(4), SKEWED_ORTHO, np.array([9.0, 12.0, 5.0]), np.array([12.0, 15.0, 8.0])))
    out.append(("huge", symmetry_atoms_xyz(2000), _operators(4), SKEWED_ORTHO, np.full(3, -1000.0), np.full(3, 1000.0)))
    return out


# ---- the point helpers ---------------------------------------------------------------------------------------------------------------
N_POINTS = 3001


def point_rows(name):
    """N_POINTS distinct raw crs rows from three intervals outside the stored grid on every side, the grid's corners among them."""
    w = world(name)
    rng = np.random.default_rng(8400 + WORLDS.index(name))
    lo = [-3 * w.interval[k] for k in range(3)]
    hi = [w.ncrs[k] + 3 * w.interval[k] for k in range(3)]
    crs = np.unique(np.stack([rng.integers(lo[k], hi[k], size=2 * N_POINTS) for k in range(3)], axis=1), axis=0)
    crs = crs[rng.permutation(len(crs))][:N_POINTS]
    corners = np.array([[c, r, s] for c in (0, w.ncrs[0] - 1) for r in (0, w.ncrs[1] - 1) for s in (0, w.ncrs[2] - 1)])
    crs[:8] = corners
    crs[8:16] = corners + np.array(w.interval) * np.array([1, -2, 3])
    assert len(np.unique(crs, axis=0)) == N_POINTS
    return np.ascontiguousarray(crs.astype(np.int32))


def point_batch_sizes(in_bytes, out_bytes):
    """Row counts of a point helper around the pinned block, from its bytes per row: the input is staged first (pinned_in), the result takes what
    is left (pinned_out); each occupies whole 64-byte lines.  -> (the largest count at which both fit; one more: the input alone; the largest at
    which the input fits; one more: the input is copied from the caller's memory; one past the result's own limit: neither uses the block)."""
    both = PINNED_BLOCK // (in_bytes + out_bytes)
    while pinned_span(in_bytes * (both + 1)) + pinned_span(out_bytes * (both + 1)) <= PINNED_BLOCK:
        both += 1
    while pinned_span(in_bytes * both) + pinned_span(out_bytes * both) > PINNED_BLOCK:
        both -= 1
    input_fits = PINNED_BLOCK // in_bytes
    neither = max(PINNED_BLOCK // in_bytes, PINNED_BLOCK // out_bytes) + 1
    sizes = [both, both + 1, input_fits, input_fits + 1, neither]
    assert in_bytes * (both + 1) > STAGED_ROW          # (an input that does not fit the block is not staged by h2d_row either)
    return sorted(set(sizes))
