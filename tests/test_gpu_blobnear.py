"""pdbeda_bloblist_nearest and the dipole table built on it, on the MI355X path against tests/blobnear_checker.py, the plain numpy
restatement of the contract in include/pdbeda.h.  The label volumes the checker reads are made from the product's own voxels()
(tests/test_gpu_voxel.py pins those bit for bit).  Every device column is an integer: every comparison is ``np.array_equal``."""
import csv
import io
import json

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import blobnear_checker as checker

pytestmark = pytest.mark.gpu

CHUNK = 2048                                   # the most list positions of one workgroup: BN_CHUNK of pdb_eda_amd/csrc/pdbeda_blobnear.h
SHORT_CHUNK = 256                              # ... and the fewest: one per thread, on lists of up to SHORT_CHUNK * MIN_GROUPS voxels
MIN_GROUPS = 512                               # a chunk doubles (to 512, 1024, CHUNK) only where that leaves this many workgroups: BN_MIN_GROUPS
SLOTS = 128                                    # blobs of a chunk whose minimum is kept in LDS: BN_SLOTS
PIECE = 4096                                   # table entries staged in LDS at a time: BN_PIECE
MAX_OFFSETS = 16384
COLUMNS = ("index", "partner", "voxel", "partnerVoxel")
_maps, _big = {}, {}


def device_map(name, gpu_ctx):
    from pdb_eda_amd import ccp4
    if name not in _maps:
        z, header, grid = load_case(name)
        _maps[name] = (header, grid, ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx))
    return _maps[name]


def synthetic_map(spec, grid, name, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=gpu_ctx)


def big_map(gpu_ctx):
    """96^3 smooth noise (the map of tests/test_gpu_blobshape.py), cut at mean +- 1 sigma."""
    from pdb_eda_amd import synthetic
    if not _big:
        spec = synthetic.MapSpec(ncrs=(96, 96, 96), spacing=0.4)
        grid = synthetic.noise_grid(spec, seed=11, sigma_voxels=1.5)
        dm = synthetic_map(spec, grid, "big", gpu_ctx)
        _big.update(dm=dm, cut=dm.meanDensity + 1.0 * dm.stdDensity)
    return _big["dm"], _big["cut"]


def labels_of(dm, bl):
    crs, off = bl.voxels()
    return checker.labels_of(dm._map.unique_shape, crs, off)


def assert_bytes_equal(a, b, what):
    for k in COLUMNS:
        assert a[k].dtype == b[k].dtype == np.int32 and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def assert_matches_checker(dm, a, b, table, what, labels=None):
    """a, b: _native.BlobList.  Returns the device columns; labels: the (a, b) volumes when the caller has made them already."""
    lab_a, lab_b = labels if labels is not None else (labels_of(dm, a), labels_of(dm, b))
    want = checker.nearest(lab_a, lab_b, table, len(a))
    got = a.nearest(b, table)
    found = int((want["index"] >= 0).sum())
    print("%s: %d blobs, %d with a partner, largest index %d of %d" % (what, len(a), found, int(want["index"].max(initial=-1)), len(table)))
    for k in COLUMNS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    return got


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_golden_maps_against_checker(gpu_ctx, name):
    from pdb_eda_amd import ccp4
    header, grid, dm = device_map(name, gpu_ctx)
    tables = {reach: ccp4.neighbourOffsets(header, reach)[0] for reach in (1.5, 2.5)}
    print("%s: %s offsets" % (name, {reach: len(t) for reach, t in tables.items()}))
    for k in (1.5, 3.0):
        cut = dm.meanDensity + k * dm.stdDensity
        green, red = dm._map.full_blobs_pm(cut, -cut)
        volumes = labels_of(dm, green), labels_of(dm, red)
        for reach, table in tables.items():
            there = assert_matches_checker(dm, green, red, table, "%s %g sigma green -> red, %g A" % (name, k, reach), volumes)
            back = assert_matches_checker(dm, red, green, table, "%s %g sigma red -> green, %g A" % (name, k, reach), volumes[::-1])
            if k == 1.5:
                found, back_found = int((there["index"] >= 0).sum()), int((back["index"] >= 0).sum())
                if reach == 1.5:                                             # (a vacuous comparison cannot pass)
                    assert found >= 5 and len(green) - found >= 1, (name, found, len(green))
                    first = found
                # the table is symmetric under o -> -o, so a red blob that is somebody's partner has one itself; a longer reach loses nobody
                assert back_found >= 1 and found >= first
                assert set(there["partner"][there["index"] >= 0].tolist()) <= set(np.nonzero(back["index"] >= 0)[0].tolist())


@pytest.mark.parametrize("name", ["orth", "hex", "wide"])
def test_separately_labelled_lists_give_the_fused_bytes(gpu_ctx, name):
    from pdb_eda_amd import ccp4
    header, grid, dm = device_map(name, gpu_ctx)
    table = ccp4.neighbourOffsets(header, 2.5)[0]
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    green, red = dm._map.full_blobs_pm(cut, -cut)
    there, back = green.nearest(red, table), red.nearest(green, table)
    assert (there["index"] >= 0).sum() >= 5
    for flag in (False, True):
        g, r = dm._map.full_blobs(cut, labels=flag), dm._map.full_blobs(-cut, labels=flag)
        assert_bytes_equal(g.nearest(r, table), there, "%s separate lists, labels=%s" % (name, flag))
        assert_bytes_equal(r.nearest(g, table), back, "%s separate lists back, labels=%s" % (name, flag))
        assert_bytes_equal(g.nearest(red, table), there, "%s separate green against the fused red, labels=%s" % (name, flag))
    fg, fr = dm._map.full_blobs_pm(cut, -cut, labels=True)
    assert_bytes_equal(fg.nearest(fr, table), there, name + " fused with a label volume")
    assert_bytes_equal(fr.nearest(fg, table), back, name + " fused with a label volume, back")
    green.free()                                                             # the red list outlives the list that owns the job's arena
    assert_bytes_equal(red.nearest(fg, table), back, name + " red after the green list has gone")


def test_blob_split_over_many_workgroups(gpu_ctx):
    from pdb_eda_amd import ccp4
    dm, cut = big_map(gpu_ctx)
    table = ccp4.neighbourOffsets(dm.header, 1.5)[0]
    green, red = dm._map.full_blobs_pm(cut, -cut)
    volumes = labels_of(dm, green), labels_of(dm, red)
    there = assert_matches_checker(dm, green, red, table, "96^3 green -> red", volumes)
    assert_matches_checker(dm, red, green, table, "96^3 red -> green", volumes[::-1])
    n = green.stats()["n"]
    print("96^3: %d green blobs, the largest of %d voxels = %.1f chunks, %d single voxels; %d offsets" % (len(n), int(n.max()), n.max() / CHUNK, int((n == 1).sum()), len(table)))
    assert n.max() > 10 * CHUNK and (n == 1).sum() >= 30
    assert (there["index"] >= 0).sum() >= 30


def test_every_chunk_size(gpu_ctx):
    """The 96^3 map lifted by half a sigma and cut near zero: a green list long enough for the largest chunk (eight positions per thread),
    a red one for the next (four) -- the golden maps, the crumbs and the 1 sigma lists above run at one or two per thread."""
    from pdb_eda_amd import ccp4, synthetic
    spec = synthetic.MapSpec(ncrs=(96, 96, 96), spacing=0.4)
    grid = synthetic.noise_grid(spec, seed=11, sigma_voxels=1.5)
    grid = (grid + np.float32(0.5 * float(grid.std()))).astype(np.float32)
    dm = synthetic_map(spec, grid, "lifted", gpu_ctx)
    cut = 0.02 * dm.stdDensity
    table = ccp4.neighbourOffsets(dm.header, 1.5)[0]
    green, red = dm._map.full_blobs_pm(cut, -cut)
    long_, short = green.voxels()[0].shape[0], red.voxels()[0].shape[0]
    print("lifted 96^3: %d green voxels in %d blobs, %d red voxels in %d blobs" % (long_, len(green), short, len(red)))
    assert long_ > 4 * SHORT_CHUNK * MIN_GROUPS and 2 * SHORT_CHUNK * MIN_GROUPS < short <= 4 * SHORT_CHUNK * MIN_GROUPS
    volumes = labels_of(dm, green), labels_of(dm, red)
    there = assert_matches_checker(dm, green, red, table, "lifted green -> red", volumes)
    back = assert_matches_checker(dm, red, green, table, "lifted red -> green", volumes[::-1])
    assert (there["index"] >= 0).any() and (back["index"] >= 0).any()


def test_run_to_run_identity(gpu_ctx):
    """Five fresh fused labellings of the 96^3 map: every column to the byte (the voxel lists themselves may differ in order)."""
    from pdb_eda_amd import ccp4
    dm, cut = big_map(gpu_ctx)
    table = ccp4.neighbourOffsets(dm.header, 1.5)[0]
    first = None
    for run in range(5):
        green, red = dm._map.full_blobs_pm(cut, -cut)
        got = green.nearest(red, table), red.nearest(green, table)
        if first is None:
            first = got
            assert (got[0]["index"] >= 0).sum() >= 5 and (got[1]["index"] >= 0).sum() >= 5
        assert_bytes_equal(got[0], first[0], "96^3 green, labelling %d" % run)
        assert_bytes_equal(got[1], first[1], "96^3 red, labelling %d" % run)


def test_chunk_of_crumbs(gpu_ctx):
    """Single voxels on a lattice of step 3: more blobs in one chunk than the LDS table holds, so the blobs beyond it take the wave
    segment's atomic directly; a few pairs of voxels among them so that segments of two lanes exist."""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(36, 30, 12), spacing=0.5)
    grid = np.zeros((12, 30, 36), dtype=np.float32)
    grid[0::3, 0::3, 0::3] = 2.0                                             # 4 x 10 x 12 = 480 green crumbs
    grid[0::6, 0::3, 1::9] = 2.0                                             # ... some of them two voxels long
    s, r, c = np.meshgrid(np.arange(12), np.arange(30), np.arange(36), indexing="ij")
    grid[(s % 3 == 1) & (r % 3 == 1) & (c % 3 == 1) & ((c // 3 + r // 3) % 3 == 0)] = -2.0          # red crumbs diagonal to a third of them
    grid[(s % 3 == 0) & (r % 6 == 0) & (c % 12 == 2) & (grid == 0)] = -2.0                         # ... and two steps along c from a few
    dm = synthetic_map(spec, grid, "crumbs", gpu_ctx)
    green, red = dm._map.full_blobs_pm(0.5, -0.5)
    for bl in (green, red):                                                  # short lists: the first chunk alone covers more blobs than the table holds
        crs, off = bl.voxels()
        assert len(crs) <= SHORT_CHUNK * MIN_GROUPS and np.searchsorted(off, SHORT_CHUNK, side="right") - 1 > SLOTS
    table = np.array([(0, 0, 0)] + [(dc, dr, ds) for dc in (-1, 0, 1) for dr in (-1, 0, 1) for ds in (-1, 0, 1) if (dc, dr, ds) != (0, 0, 0)] +
                     [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)], dtype=np.int32)
    there = assert_matches_checker(dm, green, red, table, "crumbs green -> red")
    back = assert_matches_checker(dm, red, green, table, "crumbs red -> green")
    beyond = there["index"][SLOTS:]
    assert (beyond >= 0).sum() >= 20 and (beyond < 0).sum() >= 20 and (back["index"][SLOTS:] >= 0).sum() >= 20
    assert (green.stats()["n"] == 2).sum() >= 5


def test_planted_ties(gpu_ctx):
    """Values exact in float32.  A green slab of 40 x 40 x 8 voxels (more than six chunks) with four red voxels two steps above it, so four of
    its voxels tie at one table entry across waves and workgroups: the first of them in (c, r, s) order is the answer.  A red plateau three
    steps above the slab where 150 voxels tie.  A green crumb with nobody near."""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(48, 44, 14), spacing=0.5)
    grid = np.zeros((14, 44, 48), dtype=np.float32)
    grid[2:10, 2:42, 3:43] = 2.0                                             # the slab: c 3..42, r 2..41, s 2..9; its first voxel is (3, 2, 2)
    grid[0, 0, 46] = 2.0                                                     # the crumb (46, 0, 0)
    for c, r in ((30, 7), (9, 41), (9, 12), (41, 3)):
        grid[11, r, c] = -2.0
    grid[12:14, 30:40, 5:20] = -2.0                                          # the plateau: its first voxel is (5, 30, 12)
    dm = synthetic_map(spec, grid, "ties", gpu_ctx)
    up = np.array([(0, 0, 2), (0, 0, 3), (0, 0, -2)], dtype=np.int32)
    down = np.array([(0, 0, -3), (0, 0, -2)], dtype=np.int32)
    seen = []
    for run in range(5):
        green, red = dm._map.full_blobs_pm(0.5, -0.5)
        assert green.stats()["n"].tolist() == [12800, 1] and red.stats()["n"].tolist() == [300, 1, 1, 1, 1]
        there = assert_matches_checker(dm, green, red, up, "ties green -> red, list %d" % run)
        back = assert_matches_checker(dm, red, green, down, "ties red -> green, list %d" % run)
        # red blobs in the order of their first voxels: the plateau (5, 30, 12), then (9, 12, 11), (9, 41, 11), (30, 7, 11), (41, 3, 11)
        assert there["index"].tolist() == [0, -1] and there["partner"].tolist() == [1, -1]
        assert there["voxel"].tolist() == [[9, 12, 9], [0, 0, 0]] and there["partnerVoxel"].tolist() == [[9, 12, 11], [0, 0, 0]]
        assert back["index"].tolist() == [0, 0, 0, 0, 0] and back["partner"].tolist() == [0, 0, 0, 0, 0]
        assert back["voxel"].tolist() == [[5, 30, 12], [9, 12, 11], [9, 41, 11], [30, 7, 11], [41, 3, 11]]
        assert back["partnerVoxel"].tolist() == [[5, 30, 9], [9, 12, 8], [9, 41, 8], [30, 7, 8], [41, 3, 8]]
        seen.append((there, back))
    for there, back in seen[1:]:
        assert_bytes_equal(there, seen[0][0], "ties green")
        assert_bytes_equal(back, seen[0][1], "ties red")


def test_table_sizes(gpu_ctx):
    """A table of exactly 16384 entries (four LDS pieces) on a 20^3 map with pairs whose entry lies beyond the first piece; 16385 are refused."""
    from pdb_eda_amd import _native, synthetic
    spec = synthetic.MapSpec(ncrs=(20, 20, 20), spacing=0.5)
    grid = np.zeros((20, 20, 20), dtype=np.float32)
    for c, r, s in ((0, 0, 0), (19, 19, 19), (5, 5, 5), (0, 19, 0), (6, 5, 5), (19, 0, 2)):
        grid[s, r, c] = 2.0
    for c, r, s in ((12, 12, 12), (5, 5, 8), (10, 9, 0)):
        grid[s, r, c] = -2.0
    dm = synthetic_map(spec, grid, "table", gpu_ctx)
    every = np.array([(dc, dr, ds) for dc in range(-13, 14) for dr in range(-12, 13) for ds in range(-12, 13)], dtype=np.int32)
    length = (every.astype(np.int64) ** 2).sum(axis=1)
    every = every[np.lexsort((every[:, 2], every[:, 1], every[:, 0], length))]
    assert len(every) > MAX_OFFSETS
    table = np.ascontiguousarray(every[:MAX_OFFSETS])
    green, red = dm._map.full_blobs_pm(0.5, -0.5)
    there = assert_matches_checker(dm, green, red, table, "16384 offsets green -> red")
    back = assert_matches_checker(dm, red, green, table, "16384 offsets red -> green")
    assert (there["index"] >= PIECE).sum() >= 2 and (there["index"] >= 2 * PIECE).any(), there["index"].tolist()
    assert (back["index"] >= PIECE).any()
    assert_matches_checker(dm, green, red, np.ascontiguousarray(table[:PIECE + 1]), "one entry more than a piece")
    assert_matches_checker(dm, green, red, np.ascontiguousarray(table[:PIECE]), "exactly a piece")
    gpu_ctx.profile_begin()
    with pytest.raises(_native.PdbedaError) as refusal:
        green.nearest(red, every[:MAX_OFFSETS + 1])
    assert refusal.value.code == _native.PDBEDA_ERR_ARGUMENT and not any(k.startswith("k_blobnear") for k in gpu_ctx.profile_end())
    assert_bytes_equal(green.nearest(red, table), there, "after the refusal")


def test_refusals_leave_the_context_usable(gpu_ctx):
    from pdb_eda_amd import _native, ccp4
    header, grid, dm = device_map("orth", gpu_ctx)
    other_header, _, other = device_map("hex", gpu_ctx)
    assert list(other_header.uniqueNcrs) != list(header.uniqueNcrs)
    table = ccp4.neighbourOffsets(header, 1.5)[0]
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    green, red = dm._map.full_blobs_pm(cut, -cut)
    want = green.nearest(red, table)
    assert (want["index"] >= 0).sum() >= 5
    gpu_ctx.profile_begin()
    launched = gpu_ctx.profile_end()
    assert not launched

    def refused(call):
        gpu_ctx.profile_begin()
        with pytest.raises(_native.PdbedaError) as refusal:
            call()
        launched = gpu_ctx.profile_end()
        assert refusal.value.code == _native.PDBEDA_ERR_ARGUMENT, refusal.value
        assert not any(k.startswith("k_blobnear") for k in launched), launched

    refused(lambda: green.nearest(None, table))                              # a NULL list
    refused(lambda: green.nearest(green, table))                             # a == b
    spheres = dm._map.list_blobs(np.array([[1, 1, 1], [1, 1, 2], [8, 8, 8]], dtype=np.int32))
    assert len(spheres) == 2
    refused(lambda: green.nearest(spheres, table))                           # not whole-map, either side
    refused(lambda: spheres.nearest(red, table))
    hex_cut = other.meanDensity + 1.5 * other.stdDensity
    refused(lambda: green.nearest(other._map.full_blobs(-hex_cut), table))    # unequal uniqueNcrs
    for bad in ([128, 0, 0], [0, -128, 0], [0, 0, 1000]):                    # a component outside [-127, 127], behind good entries
        refused(lambda: green.nearest(red, np.concatenate([table, np.array([bad], dtype=np.int32)])))
    edge = np.concatenate([table, np.array([[127, -127, 127]], dtype=np.int32)])
    assert_bytes_equal(green.nearest(red, edge), want, "components of +-127 are taken")
    refused(lambda: green.nearest(red, np.zeros((MAX_OFFSETS + 1, 3), dtype=np.int32)))
    refused(lambda: gpu_ctx.check(gpu_ctx._lib.pdbeda_bloblist_nearest(green._h, red._h, _native._ptr(table), -1, None, None, None, None), "pdbeda_bloblist_nearest"))   # n_offsets < 0
    second = _native.Context(gpu_ctx.device)                                 # lists of different contexts
    try:
        z, _, _ = load_case("orth")
        elsewhere = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), "orth", ctx=second)
        foreign = elsewhere._map.full_blobs(-cut)
        assert len(foreign) == len(red)
        refused(lambda: green.nearest(foreign, table))
        foreign.free()
        elsewhere._map.free()
    finally:
        second.close()
    # a freed list whose struct the other list of the fused call keeps alive
    g2, r2 = dm._map.full_blobs_pm(cut, -cut)
    handle = g2._h
    g2.free()
    out = np.zeros(len(r2), dtype=np.int32)
    lib = gpu_ctx._lib
    gpu_ctx.profile_begin()
    assert lib.pdbeda_bloblist_nearest(handle, r2._h, _native._ptr(table), len(table), None, None, None, None) == _native.PDBEDA_ERR_ARGUMENT
    assert lib.pdbeda_bloblist_nearest(r2._h, handle, _native._ptr(table), len(table), _native._ptr(out), None, None, None) == _native.PDBEDA_ERR_ARGUMENT
    assert not any(k.startswith("k_blobnear") for k in gpu_ctx.profile_end())
    with pytest.raises(_native.PdbedaError):
        g2.nearest(r2, table)
    # the context still works, and any output pointer may be NULL
    gpu_ctx.profile_begin()
    again = green.nearest(red, table)
    launched = gpu_ctx.profile_end()
    assert launched["k_blobnear_scan"][0] == 1 and launched["k_blobnear_finish"][0] == 1
    assert_bytes_equal(again, want, "after the refusals")
    only = np.zeros(len(green), dtype=np.int32)
    gpu_ctx.check(lib.pdbeda_bloblist_nearest(green._h, red._h, _native._ptr(table), len(table), None, _native._ptr(only), None, None), "pdbeda_bloblist_nearest")
    assert np.array_equal(only, want["partner"])


def test_empty_lists_and_empty_table(gpu_ctx):
    from pdb_eda_amd import ccp4
    header, grid, dm = device_map("orth", gpu_ctx)
    table = ccp4.neighbourOffsets(header, 1.5)[0]
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    top = float(np.abs(grid).max()) * 2.0
    green, nothing = dm._map.full_blobs_pm(cut, -top)
    assert len(green) >= 5 and len(nothing) == 0
    gpu_ctx.profile_begin()
    there, back = green.nearest(nothing, table), nothing.nearest(green, table)
    none = green.nearest(dm._map.full_blobs(-cut), np.zeros((0, 3), dtype=np.int32))
    assert not any(k.startswith("k_blobnear") for k in gpu_ctx.profile_end())
    for got in (there, none):
        assert got["index"].tolist() == [-1] * len(green) and got["partner"].tolist() == [-1] * len(green)
        assert not got["voxel"].any() and not got["partnerVoxel"].any() and got["voxel"].shape == (len(green), 3)
    assert all(back[k].shape[0] == 0 for k in COLUMNS) and back["voxel"].shape == (0, 3)
    lists = dm.createFullBlobLists(top)
    cols = lists[0].nearestBlobs(lists[1], 1.5)
    assert all(len(cols[k]) == 0 for k in ccp4.NEAREST_COLUMNS)


@pytest.fixture(scope="module", params=["orth", "hex"])
def analysis(request, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case(request.param)
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), request.param, ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), request.param, ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    return z, spec, st, pdb, densityAnalysis.DensityAnalysis(request.param, dens, diff, st, pdb)


def test_two_maps_on_one_grid(analysis, gpu_ctx):
    """Blue 2Fo-Fc blobs against green Fo-Fc blobs: the offset (0, 0, 0) hits where they overlap."""
    from pdb_eda_amd import ccp4
    z, spec, st, pdb, an = analysis
    dens, diff = an.densityObj, an.diffDensityObj
    blue = dens.createFullBlobList(dens.meanDensity + 1.5 * dens.stdDensity)
    green = diff.createFullBlobList(diff.meanDensity + 3.0 * diff.stdDensity)
    table, distance = ccp4.neighbourOffsets(dens.header, 2.5)
    a, b = blue._segments[0].bl, green._segments[0].bl
    volumes = labels_of(dens, a), labels_of(diff, b)
    there = assert_matches_checker(dens, a, b, table, "blue -> green", volumes)
    back = assert_matches_checker(diff, b, a, table, "green -> blue", volumes[::-1])
    overlap = (volumes[0] >= 0) & (volumes[1] >= 0)
    assert overlap.any() and (there["index"] == 0).any() and (back["index"] == 0).sum() == len(np.unique(volumes[1][overlap]))
    cols = blue.nearestBlobs(green, 2.5)
    found = there["index"] >= 0
    assert np.array_equal(cols["partner"], there["partner"]) and np.array_equal(cols["distance"][found], distance[there["index"][found]])
    assert np.isnan(cols["distance"][~found]).all() and np.array_equal(cols["voxelXyz"], dens.header.crs2xyz_array(there["voxel"]))
    assert (cols["distance"][there["index"] == 0] == 0.0).all()
    with pytest.raises(ValueError):
        (blue + blue).nearestBlobs(green, 2.5)                               # a joined list
    with pytest.raises(ValueError):
        blue.nearestBlobs(dens.createBlobList([[1, 1, 1], [1, 1, 2]]), 2.5)  # not a whole-map list
    with pytest.raises(ValueError):
        blue.nearestBlobs(green, 1e4)


def check_dipole_table(an, table, green, red, reach):
    """table: rows of blobDipoleHeader; every row recomputed from the lists' columns."""
    atoms = np.asarray(an.symmetryAtomCoords, dtype=np.float64)
    ratio = an.densityElectronRatio
    near, back = green.nearestBlobs(red, reach), red.nearestBlobs(green, reach)
    g, r = green.columns(), red.columns()
    at = 0
    for i in np.nonzero(near["partner"] >= 0)[0].tolist():
        row, j = table[at], int(near["partner"][i])
        at += 1
        assert row[0] == i and row[1] == j and row[2] == float(near["distance"][i]) and row[3] == bool(back["partner"][j] == i)
        eg, er = abs(float(g["totalDensity"][i]) / ratio), abs(float(r["totalDensity"][j]) / ratio)
        assert row[4] == eg and row[5] == er and row[6] == min(eg, er) / max(eg, er)
        shift = g["centroid"][i] - r["centroid"][j]
        middle = 0.5 * (near["voxelXyz"][i] + near["partnerVoxelXyz"][i])
        assert abs(row[7] - float(np.linalg.norm(shift))) <= 1e-12 and np.allclose(row[8], middle, rtol=0, atol=1e-12) and np.allclose(row[9], shift, rtol=0, atol=1e-12)
        d = np.sqrt(((middle[None, :] - atoms) ** 2).sum(axis=1))
        nearest = int(d.argmin())
        assert abs(row[10] - d[nearest]) <= 1e-9 and np.allclose(np.asarray(row[16], dtype=np.float64), atoms[nearest], rtol=0, atol=1e-9)
        u, v = g["centroid"][i] - atoms[nearest], r["centroid"][j] - atoms[nearest]
        assert abs(row[17] - float(u.dot(v) / (np.linalg.norm(u) * np.linalg.norm(v)))) <= 1e-12 and -1.0 - 1e-12 <= row[17] <= 1.0 + 1e-12
    assert at == len(table)
    return near


def test_dipole_table_and_mode(analysis, tmp_path):
    from pdb_eda_amd import ccp4, densityAnalysis, singleStructure
    z, spec, st, pdb, an = analysis
    diff = an.diffDensityObj
    header, table = singleStructure.rows(an, "dipole")
    assert header == densityAnalysis.DensityAnalysis.blobDipoleHeader and len(header) == 18
    green, red = diff.createFullBlobLists(diff.meanDensity + 3.0 * diff.stdDensity)
    near = check_dipole_table(an, table, green, red, 2.5)
    # the row count from the checker at 2.5 A
    offsets = ccp4.neighbourOffsets(diff.header, 2.5)[0]
    a, b = green._segments[0].bl, red._segments[0].bl
    want = checker.nearest(labels_of(diff, a), labels_of(diff, b), offsets, len(a))
    assert np.array_equal(near["partner"], want["partner"]) and np.array_equal(near["index"], want["index"])
    print("%s: %d green and %d red blobs at 3 sigma, %d dipole rows, %d mutual" % (an.pdbid, len(green), len(red), len(table), sum(row[3] for row in table)))
    assert len(table) == int((want["partner"] >= 0).sum()) and len(table) >= 3
    stats = an.calculateBlobDipoles(green, red)
    assert singleStructure.dumps(header, singleStructure._plainColumns(stats, listColumns=(15,), floatColumns=(8, 9, 16))) == singleStructure.dumps(header, table)
    short = singleStructure.rows(an, "dipole", radius=1.0)[1]
    check_dipole_table(an, short, green, red, 1.0)
    assert len(short) <= len(table) and singleStructure.rows(an, "dipole", numSD=3.0, includePdbid=True)[0][0] == "pdbid"
    top = float(np.abs(diff.density).max()) * 2.0
    assert an.calculateBlobDipoles(*diff.createFullBlobLists(top)) == []
    with pytest.raises(ValueError):
        an.calculateBlobDipoles(list(green), red)
    with pytest.raises(ValueError):
        an.calculateBlobDipoles(green + green, red)
    # both output formats through the existing writers
    back = json.loads(singleStructure.dumps(header, table, "json"))
    assert len(back) == len(table) and all(sorted(item) == sorted(header) for item in back)
    assert [item["gap_distance"] for item in back] == [row[2] for row in table] and [item["midpoint_xyz"] for item in back] == [row[8] for row in table]
    assert [item["mutual"] for item in back] == [row[3] for row in table] and [item["atom_symmetry"] for item in back] == [row[15] for row in table]
    path = tmp_path / "dipole.csv"
    singleStructure.write(header, table, str(path), "csv")
    lines = list(csv.reader(open(str(path))))
    assert lines[0] == header and len(lines) == len(table) + 1
    assert [int(line[0]) for line in lines[1:]] == [row[0] for row in table] and [float(line[2]) for line in lines[1:]] == [row[2] for row in table]


def test_planted_dipole(analysis, gpu_ctx):
    """A positive and a negative Gaussian 1.2 A either side of one atom, in an otherwise empty Fo-Fc map: exactly one row, mutual, naming that
    atom, which sits between the two blobs."""
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, an = analysis
    dens = an.densityObj
    header = dens.header
    ns, nr, nc = (int(v) for v in z["diff"].shape)
    s, r, c = np.meshgrid(np.arange(ns), np.arange(nr), np.arange(nc), indexing="ij")
    xyz = header.crs2xyz_array(np.stack([c.ravel(), r.ravel(), s.ravel()], axis=1))
    coords = np.asarray(z["atom_coord"], dtype=np.float64)
    pick = int(((coords - xyz.mean(axis=0)) ** 2).sum(axis=1).argmin())    # the atom nearest to the middle of the box
    along = np.array([1.2, 0.0, 0.0])
    grid = np.zeros(ns * nr * nc)
    for sign in (1.0, -1.0):
        grid += sign * np.exp(-((xyz - (coords[pick] + sign * along)) ** 2).sum(axis=1) / (2.0 * 0.45 ** 2))
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid.reshape(ns, nr, nc).astype(np.float32))), "planted", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    planted = densityAnalysis.DensityAnalysis("planted", dens, diff, st, pdb)
    green, red = diff.createFullBlobLists(diff.meanDensity + 3.0 * diff.stdDensity)
    assert len(green) == 1 and len(red) == 1
    table = planted.calculateBlobDipoles(green, red)
    check_dipole_table(planted, table, green, red, 2.5)
    assert len(table) == 1
    row = table[0]
    print("planted dipole: gap %.3f A, centroid distance %.3f A, atom at %.3f A from the midpoint, collinearity %.4f" % (row[2], row[7], row[10], row[17]))
    assert row[0] == 0 and row[1] == 0 and row[3] is True and row[17] < -0.9
    assert np.allclose(np.asarray(row[16], dtype=np.float64), coords[pick], rtol=0, atol=1e-6) and row[14] == str(z["atom_name"][pick])
    assert abs(row[7] - 2.4) < 0.2 and np.allclose(row[9], 2.0 * along, rtol=0, atol=0.2)
