"""Who gives a device arena back: every arena of the host library has one owner, and nothing is left lent when the last handle of a
context is freed -- after calls the library refuses, after jobs that run a second time in a larger arena, after a plain sequence.

Every test makes a context of its own, runs its sequence, frees every handle and closes the context: pdbeda_ctx_destroy returns
PDBEDA_ERR_STATE when no handle is alive and an arena is still lent (the library itself lost it), 0 otherwise.  Every failure here
is a refusal that the host library answers with a status code; nothing faults on the device."""
import ctypes as C
import io

import numpy as np
import pytest

import cloud_cases
import peaks_checker
import test_gpu_chain_order as chain_order
import test_gpu_peaks as peak_tests

pytestmark = pytest.mark.gpu

CAPACITY = -4                                    # PDBEDA_ERR_CAPACITY (include/pdbeda.h)
OFFSETS = np.array([[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2], [3, 3, 3], [-3, -3, -3]], dtype=np.int32)


def _context():
    from pdb_eda_amd import _native
    return _native.Context(0)


def _dm(spec, grid, ctx, name="ownership"):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=ctx)


def _sphere_counts(m, xyz, radii, offsets):
    bl = m.sphere_blobs(xyz, radii, offsets, 0.0)
    n = np.array(bl.stats()["n"])
    bl.free()
    return n


def test_host_sized_totals_halved(monkeypatch):
    """The inputs of test_host_sized_sphere_batches_are_checked_on_the_device: the debug hook halves the host's totals, the per-atom
    blob list fails at its first accessor and the per-atom region sums fail in the call (both hold the batch's input arena, the
    list its job arena too); the grouped call that follows answers as on a good context."""
    from pdb_eda_amd import _native, synthetic
    spec = synthetic.MapSpec(ncrs=(48, 40, 36), spacing=0.5)
    g = synthetic.smooth_noise((36, 40, 48), 5, 1.5)
    xyz = np.array([[8.0, 9.0, 7.0], [12.0, 10.5, 9.0], [15.0, 6.0, 11.0]])
    radii = np.array([1.5, 2.0, 1.5], dtype=np.float32)
    good = _context()
    dm = _dm(spec, g, good)
    want = _sphere_counts(dm._map, xyz, radii, np.array([0, 3]))
    assert len(want) >= 1
    dm._map.free()
    assert good.close() == 0
    monkeypatch.setenv("PDBEDA_DEBUG_SHRINK_TOTALS", "1")
    bad = _context()                                           # (debug hooks are read when a context is made)
    monkeypatch.delenv("PDBEDA_DEBUG_SHRINK_TOTALS")
    dm2 = _dm(spec, g, bad)
    per_atom = dm2._map.sphere_blobs(xyz, radii, np.arange(4), 0.0)
    with pytest.raises(_native.PdbedaError):
        per_atom.stats()
    per_atom.free()
    with pytest.raises(_native.PdbedaError):
        dm2._map.region_sums(xyz, radii, np.arange(4), 0.1)
    assert np.array_equal(_sphere_counts(dm2._map, xyz, radii, np.array([0, 3])), want)
    dm2._map.free()
    assert bad.close() == 0


def test_non_finite_map():
    """A 16^3 map with one NaN voxel: the sphere batch of one atom is refused by grouped_job (PDBEDA_ERR_ARGUMENT), after
    group_setup has taken the batch's input arena; the whole-map call is refused too."""
    from pdb_eda_amd import _native, synthetic
    spec = synthetic.MapSpec(ncrs=(16, 16, 16), spacing=0.5)
    g = synthetic.smooth_noise((16, 16, 16), 7, 1.5)
    g[5, 6, 7] = np.nan
    ctx = _context()
    dm = _dm(spec, g, ctx)
    with pytest.raises(_native.PdbedaError) as refusal:
        dm._map.sphere_blobs(np.array([[4.0, 4.0, 4.0]]), np.array([1.5], dtype=np.float32), np.arange(2), 0.0)
    assert refusal.value.code == _native.PDBEDA_ERR_ARGUMENT
    with pytest.raises(_native.PdbedaError):
        dm._map.full_blobs(0.5)
    dm._map.free()
    assert ctx.close() == 0


def _same_tables(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_tables(a[k], b[k]) for k in a)
    return np.array_equal(a, b, equal_nan=True) if isinstance(a, np.ndarray) else (a == b or (a != a and b != b))


def test_bad_bonded_key():
    """The crafted `chain` entry with bonded[0] = n_keys: refused (PDBEDA_ERR_ARGUMENT) while the clouds' job and the result record
    are alive.  The unmodified entry then gives, on the same context, the tables it gives on a fresh one."""
    from pdb_eda_amd import _native
    spec, header, grid, entries = cloud_cases.crafted()
    e = entries["chain"]
    fresh = _context()
    dm = cloud_cases.device_map(spec, grid, "fresh", fresh)
    want = cloud_cases.call(dm._map, e)
    assert len(want["atom"]) > 0 and len(want["res"]["residue"]) > 0
    dm._map.free()
    assert fresh.close() == 0
    ctx = _context()
    dm = cloud_cases.device_map(spec, grid, "refused", ctx)
    with pytest.raises(_native.PdbedaError) as refusal:
        cloud_cases.call(dm._map, cloud_cases.refusals(e)["bonded key out of range"])
    assert refusal.value.code == _native.PDBEDA_ERR_ARGUMENT
    got = cloud_cases.call(dm._map, e)
    assert _same_tables(got, want)
    dm._map.free()
    assert ctx.close() == 0


def test_symmetry_capacity():
    """The raw entry point: three atoms, the identity operator, a box that holds them, room for one row -- PDBEDA_ERR_CAPACITY and the
    count it needs."""
    from pdb_eda_amd._native import _ptr
    ctx = _context()
    xyz = np.array([[1.0, 1.0, 1.0], [2.0, 1.5, 1.0], [1.5, 2.5, 2.0]])
    rot = np.ascontiguousarray(np.eye(3, 4).reshape(1, 12))
    ortho = np.ascontiguousarray((10.0 * np.eye(3)).reshape(9))
    lo, hi = np.zeros(3), np.full(3, 4.0)
    idx, sym, out = np.zeros(1, np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 3))
    n = C.c_int64(-1)
    rc = ctx._lib.pdbeda_symmetry_atoms(ctx._h, _ptr(xyz), len(xyz), _ptr(rot), 1, _ptr(ortho), _ptr(lo), _ptr(hi), _ptr(idx), _ptr(sym), _ptr(out), 1, C.byref(n))
    assert rc == CAPACITY and n.value >= 3
    assert ctx.close() == 0


def test_whole_map_rerun():
    """The `rerun` grid of test_gpu_chain_order.py (one unit tile beside ordinary tiles): the fused job overflows its typical-size
    arena and runs again in the worst-case one -- the record swaps arenas -- and both lists are read in full; each against a
    single-sign job of its own, with that module's checker."""
    from pdb_eda_amd import synthetic
    g = synthetic.smooth_noise((16, 16, 128), 53, 1.5)
    cut = chain_order._noise_cut(g)
    amp = np.float32(2.0 * cut)
    g[:8, :8, 0::2] = amp
    g[:8, :8, 1::2] = -amp
    ctx = _context()
    dm = chain_order._dm(g, ctx)
    refs = {}
    for sign in (1, -1):
        bl = dm._map.full_blobs(sign * cut)
        refs[sign] = chain_order._read_all(bl, dm)
        bl.free()
    green, red = dm._map.full_blobs_pm(cut, -cut)
    for bl, sign in ((green, 1), (red, -1)):
        got = chain_order._read_all(bl, dm)
        assert got["counters"]["reruns"] == 1, got["counters"]
        chain_order._assert_same_list(got, refs[sign])
    green.free(); red.free()
    dm._map.free()
    assert ctx.close() == 0


def test_peak_search_rerun():
    """32^3 standard-normal white noise at mean + 0.0625 sigma: a local maximum per 27 voxels where the typical-size arena holds
    one per 64, so the job runs again in an arena of the size its counters name; the rows against peaks_checker, as
    test_arena_overflow_runs_the_job_again compares them."""
    ctx = _context()
    dm = peak_tests.make_dm(ctx, (32, 32, 32), seed=9, sigma_voxels=0)
    cut = dm.meanDensity + 0.0625 * dm.stdDensity
    pl = dm._map.peaks(cut)
    ctr = pl.counters()
    print("white noise 32^3 at 0.0625 sigma: %r" % (ctr,))
    assert ctr["reruns"] == 1
    peak_tests.assert_rows_equal(pl.rows(), peaks_checker.find_peaks(dm.header, dm.density, cut), "white noise 32^3")
    pl.free()
    dm._map.free()
    assert ctx.close() == 0


def plain_sequence(ctx):
    """On a 32^3 smooth-noise map: the fused whole-map lists, their peaks, basins, moments, nearest blobs, the nearest-atom partition
    and radial profiles; every handle freed.  -> what the calls returned (for a look at the sizes)"""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(32, 32, 32), spacing=0.5)
    dm = _dm(spec, synthetic.noise_grid(spec, 21, 1.5), ctx, "plain")
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    m = dm._map
    green, red = m.full_blobs_pm(cut, -cut)
    pos, neg = m.peaks_pm(cut, -cut, green, red)
    atoms = np.array([[4.0, 4.0, 4.0], [8.0, 7.5, 9.0], [12.0, 11.0, 5.0], [6.5, 13.0, 12.0]])
    out = {"blobs": (len(green), len(red)), "peaks": (len(pos), len(neg)), "basins": (pos.basins(), neg.basins(volume=True)),
           "moments": (green.moments(), red.moments()), "nearest": green.nearest(red, OFFSETS),
           "partition": m.partition(atoms, 2.0, cut), "profiles": m.radial_profiles(atoms, 2.0, 4, cut)}
    for handle in (pos, neg, green, red, m):
        handle.free()
    return out


def test_plain_sequence():
    ctx = _context()
    out = plain_sequence(ctx)
    assert min(out["blobs"]) > 0 and out["peaks"][0] >= out["blobs"][0] and out["peaks"][1] >= out["blobs"][1]
    assert len(out["basins"][0]["n"]) == out["peaks"][0] and out["basins"][1]["basin"].shape == (32, 32, 32)
    assert out["profiles"]["valid"].all() and int(out["partition"]["n"].sum()) > 0
    assert ctx.close() == 0
