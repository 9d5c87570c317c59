"""The label writer's prologue (k_labels_tiles, fused: the rank table built UNDER the second memory trip) and k_emit_tiles at the
shapes where the order of that prologue can go wrong: component ids at a tile's cap, an inbox at and beyond its cap, edge tiles,
unit tiles beside ordinary ones, maps with no blob and with one.

Every case is compared with the CPU oracle as tests/test_gpu_voxel.py compares: the label volumes of both signs equal; blob count,
n, firstKey and order equal; sums within that file's REL.  Every case runs twice in a context of its own that poisons every arena
it hands out (PDBEDA_DEBUG_POISON=1): first in a fresh arena, then, the lists freed, in the recycled one -- stale LDS, or a rank
read before its table is there, shows as a wrong label or row.
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-9   # (tests/test_gpu_voxel.py's)


@pytest.fixture
def ctx(monkeypatch):
    from pdb_eda_amd import _native
    monkeypatch.setenv("PDBEDA_DEBUG_POISON", "1")   # (read once, when the context is made)
    c = _native.Context(0)
    yield c
    c.close()


def _dm(grid, ctx):
    from pdb_eda_amd import ccp4, synthetic
    ns, nr, nc = grid.shape
    spec = synthetic.MapSpec(ncrs=(nc, nr, ns))
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "prologue", ctx=ctx)


def _oracle(dm, grid, cut):
    from oracle import oracle as ora
    o = ora.Oracle(dm.header, grid)
    return {c: o.full_blobs(c, labels=True) for c in (cut, -cut)}


def _assert_list(bl, want, shape, labels=None):
    st = bl.stats()
    assert len(bl) == len(want["n"])
    assert np.array_equal(st["n"], want["n"])
    assert np.array_equal(st["firstKey"], want["firstKey"])          # (the order of the table is the order of the first keys)
    assert np.allclose(st["totalDensity"], want["totalDensity"], rtol=REL)
    assert np.allclose(st["centroid"], want["centroid"], rtol=REL, atol=1e-9)
    assert np.allclose(st["coordCenter"], want["coordCenter"], rtol=REL, atol=1e-9)
    lab = bl.labels(shape)
    assert np.array_equal(lab, want["labels"])
    if labels is not None:
        assert np.array_equal(lab, labels)


def _check(dm, grid, cut, fused=True, single=(), emit=False):
    """Twice (fresh arena, recycled arena): the fused job, the one-sign jobs with labels (`single`: the signs), and -- `emit` -- the
    job without labels (k_emit_tiles), whose label volume is fetched afterwards and must be the fused writer's."""
    want = _oracle(dm, grid, cut)
    shape = dm._map.unique_shape
    for rep in range(2):
        lists = []
        fused_labels = None
        if fused:
            green, red = dm._map.full_blobs_pm(cut, -cut, labels=True)
            lists += [green, red]
            _assert_list(green, want[cut], shape)
            _assert_list(red, want[-cut], shape)
            fused_labels = (green.labels(shape), red.labels(shape))
        for sign in single:                                          # (one plane: key_base1 = INT64_MAX)
            one = dm._map.full_blobs(sign * cut, labels=True)
            lists.append(one)
            _assert_list(one, want[sign * cut], shape)
        if emit:
            g2, r2 = dm._map.full_blobs_pm(cut, -cut)                # no labels: k_emit_tiles ranks and writes the rows
            lists += [g2, r2]
            _assert_list(g2, want[cut], shape, fused_labels[0])      # (labels(): the non-fused writer)
            _assert_list(r2, want[-cut], shape, fused_labels[1])
        for bl in lists:
            bl.free()
    return want


# ---- component ids at the cap ----------------------------------------------------------------------------------------------

def _lattice(n, signs):
    """n isolated voxels (two apart on every axis) in ONE tile of 256 x 8 x 8, in key order, their signs taken in turn."""
    g = np.zeros((8, 8, 256), dtype=np.float32)
    pos = [(s, r, c) for s in range(0, 8, 2) for r in range(0, 8, 2) for c in range(0, 256, 2)]
    for k, (s, r, c) in enumerate(pos[:n]):
        g[s, r, c] = signs[k % len(signs)]
    return g


@pytest.mark.parametrize("n", [255, 256, 257])
def test_component_ids_at_the_cap(ctx, n):
    """255, 256 and 257 components in one tile: at 256 the tile's last id is in use, so thread 255 of the writer ranks the first
    key of volume 1 in a second pass; 257 is a wide tile (ids above the tiles' ranges).  Both signs together (fused, and each
    sign's own one-plane job), and all of one sign (fused with one list empty: the count of volume 0 is 0 or the total)."""
    for signs, single in (((1.0, -1.0), (1, -1)), ((1.0,), (1,)), ((-1.0,), (-1,))):
        g = _lattice(n, signs)
        dm = _dm(g, ctx)
        want = _check(dm, g, 0.5, single=single, emit=True)
        assert len(want[0.5]["n"]) + len(want[-0.5]["n"]) == n
        dm._map.free()


# ---- the inbox at its cap --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_tiles", [191, 192, 193, 200])
def test_inbox_at_its_cap(ctx, n_tiles):
    """A straight line, one voxel wide, along r through n_tiles tiles: every tile but the root's posts one record to the inbox of
    the root's tile -- 190, 191, 192 (= INBOX_CAP) and 199 posts; beyond the cap the posts fold with atomics.  A second, short
    blob in the root's tile has no posts: the table has a row with inbox sums and rows without.  The other sign has a line through
    three tiles and a single voxel."""
    g = np.zeros((8, 8 * n_tiles, 64), dtype=np.float32)
    g[3, :, 20] = 1.0
    g[5, 2:4, 40] = 1.0
    g[6, :24, 50] = -1.0
    g[1, 5, 10] = -1.0
    dm = _dm(g, ctx)
    want = _check(dm, g, 0.5, emit=True)
    assert sorted(int(x) for x in want[0.5]["n"]) == [2, 8 * n_tiles] and sorted(int(x) for x in want[-0.5]["n"]) == [1, 24]
    dm._map.free()


# ---- edge tiles ------------------------------------------------------------------------------------------------------------

def test_edge_tiles(ctx):
    """Noise of 70 x 21 x 19 voxels at 1.0 sigma: every tile is cut on some axis (the guarded rows), and most have an empty inbox."""
    from pdb_eda_amd import synthetic
    g = synthetic.smooth_noise((19, 21, 70), 3, 1.5)
    dm = _dm(g, ctx)
    cut = dm.meanDensity + 1.0 * dm.stdDensity
    want = _check(dm, g, cut, single=(1, -1), emit=True)
    assert len(want[cut]["n"]) > 3 and len(want[-cut]["n"]) > 3
    dm._map.free()


# ---- unit tiles beside ordinary ones -----------------------------------------------------------------------------------------

def test_unit_tile_beside_ordinary_ones(ctx):
    """2 x 2 tiles (r, s), one of them a checkerboard of both signs, sparse noise in the others and a line through all of them.
    The checkerboard tile has 8 192 word-runs, more than the 4 096 a tile's LDS tables hold, so it is a UNIT tile: the job runs a
    second time, the writer ranks that tile's roots in its rows (the table stays in LDS) and rebuilds the table at its end for the
    unit components.  (256 voxels wide: a tile of 64 x 8 x 8 voxels cannot hold more than 4 096 word-runs -- 32 a word and sign --
    and would never be a unit tile.)"""
    from pdb_eda_amd import synthetic
    ns, nr, nc = 16, 16, 256
    noise = synthetic.smooth_noise((ns, nr, nc), 19, 1.5)
    g = np.where(np.abs(noise) > 1.8, np.sign(noise), 0.0).astype(np.float32)
    g[:8, :8, :] = 0.0
    g[:8, 0:8:2, 0:256:2] = 1.0
    g[:8, 1:8:2, 1:256:2] = -1.0
    g[:, 9, 77] = 1.0                # through an ordinary tile of every s ...
    g[3, :, 100] = 1.0               # ... and from the unit tile into its r neighbour
    dm = _dm(g, ctx)
    want = _oracle(dm, g, 0.5)
    shape = dm._map.unique_shape
    for rep in range(2):
        green, red = dm._map.full_blobs_pm(0.5, -0.5, labels=True)
        _assert_list(green, want[0.5], shape)
        _assert_list(red, want[-0.5], shape)
        c = green.counters()
        assert c["unit_tiles_runs"] >= 1 and c["reruns"] >= 1, c
        one = dm._map.full_blobs(-0.5, labels=True)
        _assert_list(one, want[-0.5], shape)
        g2, r2 = dm._map.full_blobs_pm(0.5, -0.5)
        _assert_list(g2, want[0.5], shape)
        _assert_list(r2, want[-0.5], shape)
        for bl in (green, red, one, g2, r2):
            bl.free()
    dm._map.free()


# ---- nothing and one -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [(), ((4, 5, 33, 1.0),), ((4, 5, 33, -1.0),), ((0, 0, 0, 1.0),), ((8, 9, 69, -1.0),)])
def test_nothing_and_one(ctx, voxels):
    """A map without a voxel beyond the cutoff (no blob at all), and maps with exactly one -- of either sign, in the middle and in
    the first and the last voxel of the map: in the fused job one list is empty, and the count of volume 0 is 0 or the total."""
    g = np.zeros((9, 10, 70), dtype=np.float32)
    for s, r, c, v in voxels:
        g[s, r, c] = v
    dm = _dm(g, ctx)
    want = _check(dm, g, 0.5, single=(1, -1), emit=True)
    assert len(want[0.5]["n"]) == sum(1 for v in voxels if v[3] > 0) and len(want[-0.5]["n"]) == sum(1 for v in voxels if v[3] < 0)
    dm._map.free()
