"""The explicit-voxel and point entry points -- pdbeda_list_blobs (and the host fold of DeviceMap.list_stats behind DensityBlob.fromCrsList /
merge), pdbeda_test_overlap, pdbeda_symmetry_atoms, pdbeda_nearest_atom, the four point helpers and pdbeda_sum_of_abs -- on the inputs of
tests/voxelsets_cases.py: group boundaries inside a thread's share and inside a wave of k_list_boxes, empty groups, duplicates, boxes around the
64-voxel mask word, and batch sizes on both sides of the two staging limits of the host library (a staged input row of 256 KiB, the 4 MiB
pinned block that pinned_in / pinned_out hand out).

Yardsticks: the oracle (blob_list, blob_stats, test_overlap, symmetry_atoms, crs2xyz, xyz2crs), scipy's cdist and numpy; nothing comes from
the native library.  tests/test_voxelsets_host.py pins the inputs.  Every test prints the largest deviation it saw beside the bound that applied."""
import ctypes as C
import io
import types

import numpy as np
import pytest

import profiles_checker
import voxelsets_cases as cases

pytestmark = pytest.mark.gpu

REL = 1e-9          # tests/test_gpu_voxel.py


@pytest.fixture(scope="module", params=cases.WORLDS)
def world(request, gpu_ctx):
    from pdb_eda_amd import ccp4
    from oracle import oracle as ora
    w = types.SimpleNamespace(**vars(cases.world(request.param)))
    w.ctx = gpu_ctx
    w.dm = ccp4.parse(io.BytesIO(w.raw), w.name, ctx=gpu_ctx)
    w.oracle = ora.Oracle(w.header, w.grid)
    w.cache = {}
    return w


def voxel_keys(crs):
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    return ((crs[:, 0] + 4096) * 8192 + crs[:, 1] + 4096) * 8192 + crs[:, 2] + 4096


# ---- pdbeda_list_blobs ---------------------------------------------------------------------------------------------------------------
def list_want(w):
    """Per group of the full list: the oracle's blobs of np.unique(group), sorted by their sorted voxel keys -- computed once per world."""
    if "list" not in w.cache:
        want = []
        for vox in cases.list_groups(w.name).groups:
            rows = []
            for b in (w.oracle.blob_list(np.unique(vox, axis=0)) if len(vox) else []):
                rows.append(dict(b, key=np.sort(voxel_keys(b["crs"])).tobytes(), sumAbs=float(np.abs(cases.density(w, b["crs"])).sum())))
            want.append(sorted(rows, key=lambda r: r["key"]))
        w.cache["list"] = want
    return w.cache["list"]


def list_rows(m, lst):
    """The device's list: its statistics, and its voxels sorted inside every blob (the order inside a blob is not part of the contract)."""
    bl = m.list_blobs(lst.crs, lst.off)
    st = bl.stats()
    vox, voff = bl.voxels()
    out = {k: st[k].copy() for k in ("n", "totalDensity", "centroid", "coordCenter", "volume", "firstKey", "group")}
    blob_of = np.repeat(np.arange(len(voff) - 1), np.diff(voff))
    out["vox"], out["voff"] = vox[np.lexsort((voxel_keys(vox), blob_of))], voff.copy()
    bl.free()
    return out


def assert_list_equal(w, got, lst, what):
    want = list_want(w)
    n_blobs = len(got["n"])
    assert got["voff"][0] == 0 and np.array_equal(np.diff(got["voff"]), got["n"]) and got["voff"][-1] == len(got["vox"]), what
    assert np.all(np.diff(got["group"]) >= 0), what
    assert np.all((np.diff(got["firstKey"]) > 0) | (np.diff(got["group"]) > 0)), what          # strictly increasing inside a group
    sizes = np.diff(lst.off)
    assert np.array_equal(np.unique(got["group"]), np.flatnonzero(sizes > 0)), what          # an empty group has no row, every other group has one
    key = voxel_keys(got["vox"])
    starts = np.searchsorted(got["group"], np.arange(len(sizes) + 1))
    ref = [None] * n_blobs
    for g in range(len(sizes)):
        theirs = want[lst.source[g]]
        rows = sorted(range(starts[g], starts[g + 1]), key=lambda r: key[got["voff"][r]:got["voff"][r + 1]].tobytes())
        assert len(rows) == len(theirs), (what, g, lst.kind[g])
        for r, t in zip(rows, theirs):
            assert key[got["voff"][r]:got["voff"][r + 1]].tobytes() == t["key"], (what, g, lst.kind[g])          # the same voxel set
            ref[r] = t
    n = np.array([t["n"] for t in ref])
    total, volume, sum_abs = (np.array([t[k] for t in ref]) for k in ("totalDensity", "volume", "sumAbs"))
    centre, centroid = (np.array([t[k] for t in ref]).reshape(-1, 3) for k in ("coordCenter", "centroid"))
    assert np.array_equal(got["n"], n), what
    err, bound = np.abs(got["totalDensity"] - total), 1e-9 * n * w.top
    worst = int(np.argmax(err))
    print("%s: %d blobs in %d groups, %d voxels; max |totalDensity - oracle| = %.3g (bound at that blob, of %d voxels: %.3g)" %
          (what, n_blobs, len(sizes), int(n.sum()), err[worst], n[worst], bound[worst]))
    assert np.all(err <= bound), what
    for tag, mine, theirs in (("volume", got["volume"], volume), ("coordCenter", got["coordCenter"], centre)):
        print("%s: max |%s - oracle| = %.3g (bound there: %.3g)" % ((what, tag) + worst_of(mine, theirs)))
        assert np.allclose(mine, theirs, rtol=REL, atol=1e-9), (what, tag)
    # the density-weighted centroid: 0 / 0 on both sides where no voxel has density; compared where |totalDensity| >= 0.01 sum |rho|
    # (tests/test_voxelsets_host.py: fewer than 10 % of the blobs fall below that)
    none = sum_abs == 0.0
    assert np.array_equal(np.isnan(got["centroid"]).all(axis=1), none) and np.all(np.isnan(centroid[none])), what
    good = ~none & (np.abs(total) >= 0.01 * sum_abs)
    assert np.count_nonzero(good) > 0.9 * n_blobs, what
    print("%s: max |centroid - oracle| = %.3g (bound there: %.3g) over %d of %d blobs" % ((what,) + worst_of(got["centroid"][good], centroid[good]) + (np.count_nonzero(good), n_blobs)))
    assert np.allclose(got["centroid"][good], centroid[good], rtol=REL, atol=1e-9), what


def worst_of(mine, theirs, rtol=REL, atol=1e-9):
    """(the largest deviation, np.allclose's bound at that element)."""
    err, bound = np.abs(mine - theirs).reshape(-1), (atol + rtol * np.abs(theirs)).reshape(-1)
    k = int(np.argmax(err))
    return float(err[k]), float(bound[k])


def test_list_blobs_on_both_sides_of_the_staged_row(world):
    """The full list (its voxels, 12 bytes each, and its per-voxel group ids, 4 bytes each, are both beyond the 256 KiB up to which h2d_row stages
    a row: 21 845 voxels, 65 536 ids), its head (both staged) and the middle list (ids staged, voxels not) -- every blob of every group against
    the oracle's blobs of np.unique(group)."""
    w = world
    variants = cases.list_variants(w.name)
    for tag in ("full", "head", "middle"):
        lst = variants[tag]
        got = list_rows(w.dm._map, lst)
        assert_list_equal(w, got, lst, "%s %s" % (w.name, tag))
        if tag == "full":
            w.cache["full rows"] = got
            # (e): one voxel set in two groups -- the same rows but for `group`
            e1, e2 = (g for g in range(len(lst.kind)) if lst.kind[g] == "e")
            a, b = np.flatnonzero(got["group"] == e1), np.flatnonzero(got["group"] == e2)
            assert len(a) == len(b) > 0
            for k in ("n", "totalDensity", "centroid", "coordCenter", "volume", "firstKey"):
                assert got[k][a].tobytes() == got[k][b].tobytes(), k
            assert got["vox"][got["voff"][a[0]]:got["voff"][a[-1] + 1]].tobytes() == got["vox"][got["voff"][b[0]]:got["voff"][b[-1] + 1]].tobytes()
            # (f): periodic images stay two voxels of equal density
            for g in (g for g in range(len(lst.kind)) if lst.kind[g] == "f"):
                rows = np.flatnonzero(got["group"] == g)
                assert len(rows) == 2 and got["n"][rows].tolist() == [1, 1] and got["totalDensity"][rows[0]] == got["totalDensity"][rows[1]] != 0.0


def test_list_blobs_on_poisoned_arenas(world, monkeypatch):
    """The full list again on a context whose arenas are handed out filled with 0xFF (PDBEDA_DEBUG_POISON=1): the same bytes, so no kernel of the
    list job trusts recycled memory -- masks, boxes of empty groups, rank counters."""
    from pdb_eda_amd import _native, ccp4
    w = world
    lst = cases.list_groups(w.name)
    first = w.cache.get("full rows") or list_rows(w.dm._map, lst)
    monkeypatch.setenv("PDBEDA_DEBUG_POISON", "1")
    ctx = _native.Context(0)
    dm = ccp4.parse(io.BytesIO(w.raw), w.name, ctx=ctx)
    for rep in range(2):          # (the second pass runs in the arenas the first gave back)
        again = list_rows(dm._map, lst)
        assert list(again) == list(first)
        for k in first:
            assert again[k].tobytes() == first[k].tobytes(), (k, rep)
    print("%s: %d blobs, %d voxels: the same bytes on poisoned arenas, twice" % (w.name, len(first["n"]), len(first["vox"])))
    dm._map.free()
    ctx.close()


def test_from_crs_list_and_merge_fold_components(world):
    """DensityBlob.fromCrsList / merge on disconnected sets (DeviceMap.list_stats folds the components' rows on the host) against the oracle's
    blob over the whole set, rtol 1e-9; in skew also with a component of nothing but unstored voxels, whose total density is exactly 0 and
    whose own centroid is 0 / 0."""
    from pdb_eda_amd.ccp4 import DensityBlob
    w = world
    sets = cases.fold_sets(w.name)
    assert w.name == "orth" or sets[-1][0] == "zero"
    for label, a, b in sets:
        union = np.unique(np.concatenate([a, b]).astype(np.int32), axis=0)
        want = w.oracle.blob_stats(union)
        assert len(w.oracle.cluster(union)) >= 2 and np.all(np.isfinite(want["centroid"]))
        whole = DensityBlob.fromCrsList(np.concatenate([b, a]), w.dm)
        merged = DensityBlob.fromCrsList(a, w.dm)
        merged.merge(DensityBlob.fromCrsList(b, w.dm))
        for tag, blob in (("fromCrsList", whole), ("merge", merged)):
            assert blob.numVoxels == len(union) and blob.crsList == {tuple(v) for v in union.tolist()}
            mine = np.concatenate([[blob.totalDensity, blob.volume], blob.centroid, blob.coordCenter])
            theirs = np.concatenate([[want["totalDensity"], want["volume"]], want["centroid"], want["coordCenter"]])
            err = np.abs(mine - theirs)
            k = int(np.argmax(err))
            print("%s %s %s: %d voxels, max |value - oracle| = %.3g (bound there: %.3g)" % (w.name, label, tag, len(union), err[k], REL * abs(theirs[k])))
            assert np.allclose(mine, theirs, rtol=REL, atol=0), (label, tag, mine, theirs)


# ---- pdbeda_test_overlap -------------------------------------------------------------------------------------------------------------
def test_overlap_pairs_batched_and_one_by_one(gpu_ctx):
    """Sets of 0, 1, 255, 256, 257 and 1 500 voxels (the block's 256 threads walk |A| x |B|): pairs that touch at the last (a, b) of the walk
    alone, pairs that miss by 2 on one axis, a set against itself, the empty set -- all pairs in one call, and each pair in a call of its own."""
    from oracle import oracle as ora
    s = cases.overlap_sets()
    a = np.array([p[0] for p in s.pairs], dtype=np.int32)
    b = np.array([p[1] for p in s.pairs], dtype=np.int32)
    want = np.array([ora.test_overlap(s.sets[i], s.sets[j]) for i, j in zip(a, b)])
    assert 10 < np.count_nonzero(want) < len(want) - 10
    batch = gpu_ctx.test_overlap(s.crs, s.off, a, b)
    wrong = [s.pairs[p][2] for p in np.flatnonzero(batch != want)]
    print("test_overlap: %d pairs in one call, %d touching, %d wrong" % (len(want), np.count_nonzero(want), len(wrong)))
    assert not wrong, wrong
    single = np.array([gpu_ctx.test_overlap(s.crs, s.off, a[p:p + 1], b[p:p + 1])[0] for p in range(len(a))])
    wrong = [s.pairs[p][2] for p in np.flatnonzero(single != want)]
    print("test_overlap: %d pairs one by one, %d wrong" % (len(want), len(wrong)))
    assert not wrong, wrong
    # the same pairs with the sets given on their own (offsets that start at the set, as DensityBlob.testOverlap does)
    for p in (0, 9, len(a) - 1):
        A, B = s.sets[a[p]], s.sets[b[p]]
        if len(A) and len(B):
            assert gpu_ctx.test_overlap(np.concatenate([A, B]), [0, len(A), len(A) + len(B)], [0], [1])[0] == want[p]


# ---- pdbeda_nearest_atom -------------------------------------------------------------------------------------------------------------
def assert_nearest(got, first, nearest, what):
    gi, gd = got
    assert np.array_equal(gi, first), (what, np.flatnonzero(gi != first)[:5])
    rel = np.abs(gd - nearest) / np.where(nearest > 0, nearest, 1.0)
    print("%s: %d centroids, max relative |distance - cdist| = %.3g (bound 1e-15)" % (what, len(gi), rel.max()))
    assert np.allclose(gd, nearest, rtol=1e-15, atol=0), what


def test_nearest_atom_ties_take_the_first_index(gpu_ctx):
    """1, 255, 256, 257, 1 000 and 12 000 atoms (12 000 x 24 bytes: beyond the staged row) with duplicated atoms 1, 256 and 256 k + 3 indices
    apart -- ties inside one thread's stride of 256 and across threads -- and centroids mirrored between two atoms: np.argmin(cdist), the
    first index, on every row; the distance as cdist's."""
    from scipy.spatial.distance import cdist
    for case in cases.nearest_cases():
        d = cdist(case.centroids, case.atoms)
        got = gpu_ctx.nearest_atom(case.centroids, case.atoms)
        assert_nearest(got, np.argmin(d, axis=1), d.min(axis=1), "%d atoms" % len(case.atoms))
        for row, lo, hi, what in case.ties:
            assert d[row, lo] == d[row, hi] and got[0][row] == lo, (len(case.atoms), what, got[0][row])
        assert len(case.ties) >= 2 or len(case.atoms) == 1


def test_nearest_atom_around_the_pinned_block(gpu_ctx):
    """Against 300 atoms, centroid counts from cases.nearest_batch_sizes(): 262 144 (index and distance, 8 bytes a centroid each, fill the 4 MiB
    block exactly: both are written straight into it), 262 145 (the index fits, the distance is copied from device memory), 524 288 (the index
    fills the block alone) and 524 289 (neither fits).  About 3 000 distinct centroids, ties among them, expanded by index; every row compared."""
    from scipy.spatial.distance import cdist
    case = cases.nearest_case(300, n_random=2990)
    p = len(case.centroids)
    assert p > 2990 and len(case.ties) >= 6 and len(np.unique(case.centroids, axis=0)) == p
    d = cdist(case.centroids, case.atoms)
    first, nearest = np.argmin(d, axis=1), d.min(axis=1)
    for row, lo, hi, what in case.ties:
        assert d[row, lo] == d[row, hi] == nearest[row] and first[row] == lo
    for n in cases.nearest_batch_sizes():
        idx = np.arange(n) % p
        got = gpu_ctx.nearest_atom(case.centroids[idx], case.atoms)
        assert_nearest(got, first[idx], nearest[idx], "%d centroids x 300 atoms" % n)


# ---- pdbeda_symmetry_atoms -----------------------------------------------------------------------------------------------------------
def test_symmetry_atoms_against_the_oracle(gpu_ctx):
    """1, 2 and 4 operators on a skewed cell, candidate counts that fill neither a 64-bit keep word nor a block, a tight box, and 216 000
    survivors (their coordinates, 5.2 MB, do not fit the pinned block: copied from device memory): indices and symmetry quadruples equal the
    oracle's, coordinates within 1e-12; the rows of the large call that a call on the first 333 atoms also makes are the same bits."""
    from oracle import oracle as ora
    for label, xyz, rot, ortho, lo, hi in cases.symmetry_cases():
        want = ora.symmetry_atoms(xyz, rot, ortho, lo, hi)
        got = gpu_ctx.symmetry_atoms(xyz, rot, ortho, lo, hi)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
        print("symmetry %s: %d of %d images kept, max |xyz - oracle| = %.3g (bound 1e-12)" % (label, len(want[0]), 27 * len(rot) * len(xyz), np.abs(got[2] - want[2]).max()))
        assert np.allclose(got[2], want[2], rtol=0, atol=1e-12), label
        if label == "huge":
            few = 333
            small = gpu_ctx.symmetry_atoms(xyz[:few], rot, ortho, lo, hi)
            t = np.arange(27 * len(rot) * few)
            rows = (t // few) * len(xyz) + t % few          # candidate order: (cell, operator, atom), and every candidate survives
            assert len(small[0]) == len(t) and np.array_equal(got[0][rows], small[0]) and np.array_equal(got[1][rows], small[1])
            assert got[2][rows].tobytes() == small[2].tobytes()


def test_symmetry_atoms_reports_the_capacity_it_needs(gpu_ctx):
    """Through the C entry point: cap one below the need is PDBEDA_ERR_CAPACITY with n_out = the need and nothing written past cap; the context
    answers the next call as before."""
    from oracle import oracle as ora
    from pdb_eda_amd._native import _ptr
    label, xyz, rot, ortho, lo, hi = cases.symmetry_cases()[2]
    ortho = np.ascontiguousarray(ortho, dtype=np.float64).reshape(9)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    want = ora.symmetry_atoms(xyz, rot, ortho, lo, hi)
    need = len(want[0])
    assert 1 < need < 27 * len(rot) * len(xyz)

    def call(cap):
        idx, sym, out = np.full(need, -7, dtype=np.int32), np.full((need, 4), -7, dtype=np.int32), np.full((need, 3), -7.0)
        n = C.c_int64(-1)
        rc = gpu_ctx._lib.pdbeda_symmetry_atoms(gpu_ctx._h, _ptr(xyz), len(xyz), _ptr(rot), len(rot), _ptr(ortho), _ptr(lo), _ptr(hi), _ptr(idx), _ptr(sym), _ptr(out), cap, C.byref(n))
        return rc, n.value, idx, sym, out

    rc, n, idx, sym, out = call(need - 1)
    print("symmetry capacity: cap %d, status %d, n_out %d (need %d)" % (need - 1, rc, n, need))
    assert rc == -4 and n == need          # PDBEDA_ERR_CAPACITY
    assert idx[-1] == -7 and np.all(sym[-1] == -7) and np.all(out[-1] == -7.0)
    assert b"capacity" in gpu_ctx._lib.pdbeda_last_error(gpu_ctx._h)
    rc, n, idx, sym, out = call(need)
    assert rc == 0 and n == need and np.array_equal(idx, want[0]) and np.array_equal(sym, want[1]) and np.allclose(out, want[2], rtol=0, atol=1e-12)
    again = gpu_ctx.symmetry_atoms(xyz, rot, ortho, lo, hi)
    assert np.array_equal(again[0], want[0]) and again[2].tobytes() == out.tobytes()


# ---- the point helpers -----------------------------------------------------------------------------------------------------------------
def test_point_helpers_around_the_pinned_block(world):
    """3 001 distinct crs rows up to three intervals outside the grid, expanded by index to cases.point_batch_sizes(bytes in, bytes out) rows per
    helper: the largest count at which input and result both fit the 4 MiB block, one more (the input alone is staged there), the largest
    count whose input fits, one more (the input is copied from the caller's memory, the result may still use the block), and one past the
    larger of the two limits (neither uses it).  Bytes a row: point_density 12 in / 8 out, valid_crs 12 / 1, crs2xyz 12 / 24, xyz2crs 24 / 12.
    point_density and valid_crs against the numpy wrap rule; crs2xyz and xyz2crs bit-exact against the oracle."""
    w = world
    m = w.dm._map
    rows = cases.point_rows(w.name)
    rho, ok = profiles_checker.point_density(w.header, w.grid, rows.astype(np.int64))
    assert ok.any() and (w.name == "orth" or not ok.all()) and np.count_nonzero(rho) > 100
    xyz = np.array([w.oracle.crs2xyz(v) for v in rows])
    rng = np.random.default_rng(8300)
    xyz32 = np.concatenate([rng.uniform(xyz.min(axis=0), xyz.max(axis=0), size=(len(rows) - 500, 3)), xyz[:500]]).astype(np.float32).astype(np.float64)
    back = np.array([w.oracle.xyz2crs(p) for p in xyz32], dtype=np.int32)
    assert np.count_nonzero(np.all(back[-500:] == rows[:500], axis=1)) == 500          # (a voxel centre rounded to float32 still rounds to its voxel)
    for name, call, src, want, per_row in (("point_density", m.point_density, rows, rho, (12, 8)), ("valid_crs", m.valid_crs, rows, ok, (12, 1)),
                                           ("crs2xyz", m.crs2xyz, rows, xyz, (12, 24)), ("xyz2crs", m.xyz2crs, xyz32, back, (24, 12))):
        for n in [len(src)] + cases.point_batch_sizes(*per_row):
            idx = np.arange(n) % len(src)
            got = call(src[idx])
            wrong = np.flatnonzero(np.any((got != want[idx]).reshape(n, -1), axis=1))
            print("%s %s: %d rows, %d differ from the yardstick (bound 0)" % (w.name, name, n, len(wrong)))
            assert got.dtype == want.dtype and len(wrong) == 0, (name, n, wrong[:5])


# ---- pdbeda_sum_of_abs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 3, 5, 9, 17, 33, 129, 1025, 3100])
def test_sum_of_abs_is_strict_on_every_tail_shape(gpu_ctx, n_rows):
    """Grids of 1 x n_rows x 11 voxels (tails of 0 to 3 voxels behind the float4 part of k_reduce_partials): sum |v| over |v| > cutoff, strict --
    a cutoff that IS one voxel's |v| leaves that voxel out, in the float4 part and in the tail; cutoff 0; a cutoff above the maximum gives
    exactly 0.  Against numpy in fp64 at rel 1e-12."""
    from pdb_eda_amd import ccp4, synthetic
    rng = np.random.default_rng(2000 + n_rows)
    g32 = (rng.standard_normal((1, n_rows, 11)) * 3.0 + 0.7).astype(np.float32)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(synthetic.MapSpec(ncrs=(11, n_rows, 1)), g32)), "abs", ctx=gpu_ctx)
    a32, a64 = np.abs(g32).reshape(-1), np.abs(g32.astype(np.float64)).reshape(-1)
    picks = {"a voxel of the float4 part": a32[(a32.size // 2) & ~3], "the last voxel": a32[-1], "the smallest |v|": a32.min(), "the largest |v|": a32.max()}
    worst = 0.0
    for what, cut in list(picks.items()) + [("zero", np.float32(0.0)), ("between", np.float32(2.0)), ("above the maximum", np.nextafter(a32.max(), np.float32(np.inf)))]:
        want = float(a64[a32 > np.float32(cut)].sum())
        got = dm._map.sum_of_abs(float(cut))
        if what in picks:          # the voxel at the cutoff is what a >= would add
            assert np.count_nonzero(a32 >= cut) > np.count_nonzero(a32 > cut) and float(cut) > 1e-10 * max(want, 1.0)          # (a hundred times the bound)
        if want == 0.0:
            assert got == 0.0, (what, got)
        else:
            worst = max(worst, abs(got - want) / want)
            assert got == pytest.approx(want, rel=1e-12), (what, cut)
        assert dm.getTotalAbsDensity(float(cut)) == got
    assert dm._map.sum_of_abs(float(a32.max())) == 0.0 and dm._map.sum_of_abs(0.0) == pytest.approx(float(a64.sum()), rel=1e-12)
    print("sum_of_abs %d voxels (tail %d): max relative |sum - numpy| = %.3g (bound 1e-12)" % (a32.size, a32.size % 4, worst))
