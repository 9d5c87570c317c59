"""The load chains of k_face_merge and k_resolve_tiles (and the job's unit flag, which k_face_merge reads in its first trip
for its cold tail): every path behind the statements whose ORDER the chains depend on, against the CPU oracle.

A change of order in these kernels cannot change a result by design -- the stores and paints of k_resolve_tiles are fire and
forget, the flag is written by an earlier kernel -- so what can go wrong is a path that no longer runs: a tile of roots only
that returns before it paints, a post that is lost behind the inbox's cap, a job with a unit tile that no longer flags
itself.  Each case is a fused green / red job with labels, compared with the oracle in table order, voxel membership and
label volume, and run twice: the two runs must agree to the bit."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-9
STAT_KEYS = ("n", "firstKey", "totalDensity", "centroid", "coordCenter", "volume")


def _dm(grid, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic
    ns, nr, nc = grid.shape
    spec = synthetic.MapSpec(ncrs=(nc, nr, ns))
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "chain", ctx=gpu_ctx)


def _run(dm, cut):
    green, red = dm._map.full_blobs_pm(cut, -cut, labels=True)
    out = []
    for bl in (green, red):
        st = bl.stats()
        crs, off = bl.voxels()
        out.append({"stats": {k: np.array(st[k]) for k in STAT_KEYS}, "crs": np.array(crs), "off": np.array(off),
                    "labels": np.array(bl.labels(dm._map.unique_shape)), "counters": bl.counters()})
    green.free(); red.free()
    return out


def _check(grid, gpu_ctx, cut):
    """Both lists of the job against the oracle, and a second run of the job against the first.  -> the first run's outputs"""
    from oracle import oracle as ora
    dm = _dm(grid, gpu_ctx)
    o = ora.Oracle(dm.header, grid)
    first, second = _run(dm, cut), _run(dm, cut)
    for got, c in zip(first, (cut, -cut)):
        want = o.full_blobs(c, labels=True)
        st = got["stats"]
        # the blob table, in the reference's emission order
        assert np.array_equal(st["n"], want["n"])
        assert np.array_equal(st["firstKey"], want["firstKey"])
        assert np.allclose(st["totalDensity"], want["totalDensity"], rtol=REL)
        assert np.allclose(st["centroid"], want["centroid"], rtol=REL, atol=1e-9)
        assert np.allclose(st["coordCenter"], want["coordCenter"], rtol=REL, atol=1e-9)
        # the label volume
        assert np.array_equal(got["labels"], want["labels"])
        # voxel membership: blob k's voxel list is the set of voxels the oracle labels k
        crs, off = got["crs"], got["off"]
        assert off[-1] == want["n"].sum()
        assert np.array_equal(want["labels"][crs[:, 2], crs[:, 1], crs[:, 0]], np.repeat(np.arange(len(want["n"])), want["n"]))
    for a, b in zip(first, second):
        for k in STAT_KEYS:
            assert a["stats"][k].tobytes() == b["stats"][k].tobytes(), k
        assert np.array_equal(a["labels"], b["labels"])
        assert np.array_equal(a["off"], b["off"])
        assert np.array_equal(_sorted_lists(a), _sorted_lists(b))   # (a blob's voxels as a set: their order inside a list is not part of the contract)
    return first


def _sorted_lists(run):
    """The voxel lists with every blob's voxels in key order (the order inside a list follows the order of atomics)."""
    crs, off = run["crs"].astype(np.int64), run["off"]
    blob = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.lexsort((crs[:, 0], crs[:, 1], crs[:, 2], blob))
    return crs[order]


def _noise_cut(g, nsd=1.5):
    return float(np.mean(g, dtype=np.float64)) + nsd * float(np.std(g.astype(np.float64)))


def test_one_tile_column(gpu_ctx):
    """64 x 24 x 24 (c x r x s) smooth noise at +-1.5 sigma: 3 x 3 tiles in one tile column.  Tiles that hold roots only (the
    resolve pass has nothing to post there, and must still store and paint), tiles with members, posts across tiles."""
    from pdb_eda_amd import synthetic
    g = synthetic.smooth_noise((24, 24, 64), 51, 1.5)
    out = _check(g, gpu_ctx, _noise_cut(g))
    assert len(out[0]["stats"]["n"]) > 3 and len(out[1]["stats"]["n"]) > 3
    assert out[0]["counters"]["unit_tiles_runs"] + out[0]["counters"]["unit_tiles_comps"] == 0 and out[0]["counters"]["reruns"] == 0


def test_two_tile_columns(gpu_ctx):
    """320 x 16 x 16 smooth noise: two tile columns -- the 512-thread face merge with its c faces."""
    from pdb_eda_amd import synthetic
    g = synthetic.smooth_noise((16, 16, 320), 52, 1.5)
    out = _check(g, gpu_ctx, _noise_cut(g))
    lab = out[0]["labels"]
    crossing = np.intersect1d(lab[:, :, 255][lab[:, :, 255] >= 0], lab[:, :, 256][lab[:, :, 256] >= 0])
    assert crossing.size > 0                     # some green blob really crosses the c face
    assert out[0]["counters"]["reruns"] == 0


def test_spanning_blob_overflows_the_inbox(gpu_ctx):
    """64 x 136 x 136, zero but for ONE connected green lattice that enters each of the 289 tiles, and one isolated two-voxel
    green blob and one red voxel in every tile: 288 tiles post to the tile that owns the lattice's root -- more than its inbox
    holds (192), so the posts behind the cap take the atomic fold -- and every tile owns a root of its own."""
    ns = nr = 136
    g = np.zeros((ns, nr, 64), dtype=np.float32)
    g[:, 4::8, 10] = 1.0          # a line along s through every tile row ...
    g[3, :, 10] = 1.0             # ... tied together along r
    g[6::8, 1::8, 40:42] = 1.0    # the tiles' own blobs (far from the lattice and from each other)
    g[1::8, 6::8, 50] = -1.0
    out = _check(g, gpu_ctx, 0.5)
    n_green = out[0]["stats"]["n"]
    assert len(n_green) == 1 + 17 * 17 and n_green.max() == int((g[:, :, 10] > 0).sum())
    assert sorted(n_green.tolist())[:-1] == [2] * (17 * 17)
    assert out[1]["stats"]["n"].tolist() == [1] * (17 * 17)
    assert out[0]["counters"]["reruns"] == 0


def test_unit_tile_beside_ordinary_tiles(gpu_ctx):
    """128 x 16 x 16: one tile is a two-sign checkerboard along c (8 192 word-runs: more than a tile holds in LDS -- a unit
    tile), its three neighbours smooth noise.  The job flags itself (k_face_merge reads the unit flag in its first trip and
    parks it for its tail; the fused label writer reads it behind its rows) and runs again with the unit launches: the
    oracle's answer, `reruns` = 1."""
    from pdb_eda_amd import synthetic
    g = synthetic.smooth_noise((16, 16, 128), 53, 1.5)
    cut = _noise_cut(g)
    amp = np.float32(2.0 * cut)
    g[:8, :8, 0::2] = amp
    g[:8, :8, 1::2] = -amp
    out = _check(g, gpu_ctx, cut)
    for run in out:
        c = run["counters"]
        assert c["unit_tiles_runs"] + c["unit_tiles_comps"] > 0, c      # the fallback path really ran
        assert c["reruns"] == 1, c                                      # ... as the second run of its job


# ---- the lifetime of a fused job's two lists ----------------------------------------------------------------------------
# One list of a fused green / red call is freed while the other is still read.  What the survivor reads -- its part of the
# job's blob table, the job's voxel lists, the label volume written on demand, its moment rows -- is compared with a
# separate single-sign job on the same map: the same columns to the byte (`group`, the list's plane inside its job, is 1
# for the red list of a fused job and 0 for a job of its own: not compared), the same labels, the same voxels per blob.
MOMENT_KEYS = ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2", "sw", "sw1", "sw2")
_lifetime_refs = {}


def _lifetime_case(name, gpu_ctx):
    """-> (map, cut, {sign: what a separate full_blobs(sign * cut) reads}); made once per grid and left unchanged"""
    if name not in _lifetime_refs:
        from pdb_eda_amd import synthetic
        if name == "rerun":          # the grid of test_unit_tile_beside_ordinary_tiles
            g = synthetic.smooth_noise((16, 16, 128), 53, 1.5)
            cut = _noise_cut(g)
            amp = np.float32(2.0 * cut)
            g[:8, :8, 0::2] = amp
            g[:8, :8, 1::2] = -amp
        else:                        # the grid of test_one_tile_column
            g = synthetic.smooth_noise((24, 24, 64), 51, 1.5)
            cut = _noise_cut(g)
        dm = _dm(g, gpu_ctx)
        refs = {}
        for sign in (1, -1):
            bl = dm._map.full_blobs(sign * cut)
            refs[sign] = _read_all(bl, dm)
            bl.free()
        _lifetime_refs[name] = (dm, cut, refs)
    return _lifetime_refs[name]


def _read_all(bl, dm, what=("len", "stats", "voxels", "labels", "moments", "counters")):
    out = {}
    if "len" in what:
        out["len"] = len(bl)
    if "stats" in what:
        st = bl.stats()
        out["stats"] = {k: np.array(st[k]) for k in STAT_KEYS}
    if "voxels" in what:
        crs, off = bl.voxels()
        out["crs"], out["off"] = np.array(crs), np.array(off)
    if "labels" in what:
        out["labels"] = np.array(bl.labels(dm._map.unique_shape))
    if "moments" in what:
        mo = bl.moments()
        out["moments"] = {k: np.array(mo[k]) for k in MOMENT_KEYS}
    if "counters" in what:
        out["counters"] = bl.counters()
    return out


def _assert_same_list(got, want):
    if "len" in got:
        assert got["len"] == want["len"] and got["len"] > 0
    if "stats" in got:
        for k in STAT_KEYS:
            assert got["stats"][k].tobytes() == want["stats"][k].tobytes(), k
    if "moments" in got:
        for k in MOMENT_KEYS:
            assert got["moments"][k].tobytes() == want["moments"][k].tobytes(), k
    if "labels" in got:
        assert np.array_equal(got["labels"], want["labels"])
    if "crs" in got:
        assert np.array_equal(got["off"], want["off"])
        assert np.array_equal(_sorted_lists(got), _sorted_lists(want))


@pytest.mark.parametrize("name,reruns", [("rerun", 1), ("plain", 0)])
def test_green_freed_before_any_accessor(gpu_ctx, name, reruns):
    """A fused job without a label volume; the green list is freed before anything was read, then the red list is read in
    full: on the map whose job runs again (the survivor alone moves to the second run) and on one whose job does not."""
    dm, cut, refs = _lifetime_case(name, gpu_ctx)
    green, red = dm._map.full_blobs_pm(cut, -cut)
    green.free()
    got = _read_all(red, dm)
    red.free()
    assert got["counters"]["reruns"] == reruns, got["counters"]
    _assert_same_list(got, refs[-1])


def test_red_freed_before_any_accessor(gpu_ctx):
    """The mirror image on the map whose job runs again: the red list goes first, the green list is read."""
    dm, cut, refs = _lifetime_case("rerun", gpu_ctx)
    green, red = dm._map.full_blobs_pm(cut, -cut)
    red.free()
    got = _read_all(green, dm)
    green.free()
    assert got["counters"]["reruns"] == 1, got["counters"]
    _assert_same_list(got, refs[1])


def test_list_freed_between_the_rerun_and_the_voxel_lists(gpu_ctx):
    """len(green) runs the job again; green is freed; the voxel lists and the moment rows are then made for red alone."""
    dm, cut, refs = _lifetime_case("rerun", gpu_ctx)
    green, red = dm._map.full_blobs_pm(cut, -cut)
    assert len(green) == refs[1]["len"]
    green.free()
    got = _read_all(red, dm, what=("voxels", "moments", "counters"))
    red.free()
    assert got["counters"]["reruns"] == 1, got["counters"]
    _assert_same_list(got, refs[-1])
