"""pdbeda_map_spread on the MI355X path against tests/spread_checker.py, the plain numpy restatement of the contract in include/pdbeda.h -- TO THE
BIT: the contract is integer up to the value's lookup and a lane owns its voxel, so the float32 maps are compared as uint32 (without a base a
NaN among the values keeps its payload; with one, where the checker's product is a NaN only the NaN-ness is compared).  With values[t] = t the
ranks themselves are compared.  tests/test_spread_host.py holds the checker against scipy and guards that no compared case is trivial;
tests/test_spread_plan_host.py holds the host plan."""
import io
import os

import numpy as np
import pytest

import spread_cases as cases
import spread_checker as checker

pytestmark = pytest.mark.gpu

_maps, _wanted = {}, {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_map(gpu_ctx, geometry, data, tag):
    from pdb_eda_amd import ccp4, synthetic
    key = (geometry, tag)
    if key not in _maps:
        _maps[key] = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(cases.spec_of(geometry), data)), geometry, ctx=gpu_ctx)
    return _maps[key]


def seeded(gpu_ctx, geometry, seeds):
    x, threshold, below = cases.grid(seeds, geometry)
    return device_map(gpu_ctx, geometry, x, seeds), x, threshold, below


def wanted(key, make):
    if key not in _wanted:
        _wanted[key] = make()
    return _wanted[key]


def assert_same_bits(got, want, what, nan_as_nan=False):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    differ = got.view(np.uint32) != want.view(np.uint32)
    if nan_as_nan:
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        differ &= ~np.isnan(want)
    if differ.any():
        at = tuple(int(v[0]) for v in np.nonzero(differ))
        print("%s: %d of %d voxels differ, first at [s][r][c] = %s: got %r, want %r" % (what, int(differ.sum()), got.size, at, float(got[at]), float(want[at])))
    assert not differ.any(), what


def run_case(gpu_ctx, case, monkeypatch=None, rows=True):
    tag, geometry, table, seeds, with_base, kind = case
    offsets, compilable = cases.table(table, geometry)
    dm, x, threshold, below = seeded(gpu_ctx, geometry, seeds)
    values = cases.values_of(len(offsets), kind)
    base_grid = cases.base_of(geometry) if with_base else None
    base = device_map(gpu_ctx, geometry, base_grid, "base") if with_base else None
    iv = cases.intervals_of(geometry)
    want = wanted(("spread", tag), lambda: checker.spread(x, offsets, values, iv, threshold, below, base_grid))
    if monkeypatch is not None:
        monkeypatch.setenv("PDBEDA_SPREAD_ROWS", "1" if rows else "0")
    out, ctr = dm.spread(offsets, values, threshold, below, base, counters=True)
    assert list(out.header.ncrs) == list(dm.header.ncrs)
    assert_same_bits(out.density, want, tag, nan_as_nan=with_base)
    assert (ctr["seeds"], ctr["reached"]) == wanted(("counters", tag), lambda: checker.counters(x, offsets, iv, threshold, below)), tag
    assert ctr["rows"] == (1 if (compilable and rows) else 0), tag
    return out.density


@pytest.mark.parametrize("case", cases.compared_cases(), ids=lambda c: c[0])
def test_spread_against_checker(gpu_ctx, case):
    """Every geometry, table and kind of seeds of tests/spread_cases.py: the map to the bit, the two counts, and the path the table takes."""
    run_case(gpu_ctx, case)


@pytest.mark.parametrize("case", [c for c in cases.compared_cases() if cases.table(c[2], c[1])[1]], ids=lambda c: c[0])
def test_rows_against_the_forced_walk(gpu_ctx, case, monkeypatch):
    """PDBEDA_SPREAD_ROWS=0 is read at every call: the same table walked in order gives the same bits (and says so in its counters)."""
    walked = run_case(gpu_ctx, case, monkeypatch, rows=False)
    by_rows = run_case(gpu_ctx, case, monkeypatch, rows=True)
    assert np.array_equal(walked.view(np.uint32), by_rows.view(np.uint32))


def test_largest_ball(gpu_ctx):
    """The largest ball of spreadTable within 16384 offsets on a 40 x 36 x 32 map with two seeds: the ranks to the bit, by rows and walked."""
    offsets, distance, radius = cases.largest_ball()
    assert 16000 < len(offsets) <= cases.MAX_OFFSETS
    x = np.zeros(cases.shape_of("big"), dtype=np.float32)
    x[3, 30, 7] = x[20, 5, 33] = 1.0
    dm = device_map(gpu_ctx, "big", x, "two-seeds")
    values = cases.values_of(len(offsets))
    want = checker.spread(x, offsets, values, cases.intervals_of("big"))
    reached = float((want < len(offsets)).mean())
    assert 0.05 <= reached <= 0.95
    out, ctr = dm.spread(offsets, values, counters=True)
    assert_same_bits(out.density, want, "largest ball")
    assert ctr == {"seeds": 2, "reached": int((want < len(offsets)).sum()), "rows": 1}
    os.environ["PDBEDA_SPREAD_ROWS"] = "0"
    try:
        walked, ctr = dm.spread(offsets, values, counters=True)
    finally:
        del os.environ["PDBEDA_SPREAD_ROWS"]
    assert ctr["rows"] == 0
    assert_same_bits(walked.density, want, "largest ball, walked")


def test_two_calls_agree(gpu_ctx):
    case = [c for c in cases.compared_cases() if c[0] == "two-ball25-noise2"][0]
    assert np.array_equal(run_case(gpu_ctx, case).view(np.uint32), run_case(gpu_ctx, case).view(np.uint32))


def test_tile_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_spreadplan.h")).read()
    for name, value in (("SP_TILE_C", cases.TILE[0]), ("SP_TILE_R", cases.TILE[1]), ("SP_TILE_S", cases.TILE[2]), ("SP_MAX_OFFSETS", cases.MAX_OFFSETS),
                        ("SP_MAX_REACH", cases.MAX_REACH)):
        assert "constexpr int %s = %d;" % (name, value) in text
    header = open(os.path.join(ROOT, "include", "pdbeda.h")).read()
    assert "#define PDBEDA_SPREAD_MAX_OFFSETS %d" % cases.MAX_OFFSETS in header and "#define PDBEDA_SPREAD_MAX_REACH %d" % cases.MAX_REACH in header


def test_refusals_leave_the_context_usable(gpu_ctx):
    """Every refusal of the contract raises before any launch; the next call on the same context works."""
    from pdb_eda_amd import _native
    dm, x, threshold, below = seeded(gpu_ctx, "box", "noise30")
    other = seeded(gpu_ctx, "tile", "noise2")[0]
    ball = cases.table("ball10", "box")[0]
    values = cases.values_of(len(ball))
    raw = dm._map

    def refused(call):
        with pytest.raises(_native.PdbedaError) as info:
            call()
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT

    far = ball.copy()
    far.setflags(write=True)
    for k in range(3):
        for v in (33, -33):
            o = far.copy()
            o[-1, k] = v
            refused(lambda: raw.spread(o, values))
    refused(lambda: raw.spread(np.zeros((cases.MAX_OFFSETS + 1, 3), dtype=np.int32), np.zeros(cases.MAX_OFFSETS + 2, dtype=np.float32)))
    refused(lambda: raw.spread(np.zeros((0, 3), dtype=np.int32), np.zeros(1, dtype=np.float32)))
    refused(lambda: raw.spread(ball, values, threshold=float("nan")))
    refused(lambda: raw.spread(ball, values, base=other._map))
    lib, h = gpu_ctx._lib, _native.C.c_void_p()
    ptr = lambda a: a.ctypes.data_as(_native.C.c_void_p)
    args = lambda **kw: [kw.get("map", raw._h), _native.C.c_float(0.5), kw.get("flags", 0), kw.get("offsets", ptr(ball)), len(ball), kw.get("values", ptr(values)), None,
                         kw.get("out", _native.C.byref(h)), None]
    for bad in (dict(flags=2), dict(flags=0x80000000), dict(map=None), dict(offsets=None), dict(values=None), dict(out=None)):
        assert lib.pdbeda_map_spread(*args(**bad)) == _native.PDBEDA_ERR_ARGUMENT
        assert not h.value
    try:
        other_ctx = _native.Context(0)
    except _native.PdbedaError:
        other_ctx = None
    if other_ctx is not None:
        from pdb_eda_amd import ccp4, synthetic
        foreign = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(cases.spec_of("box"), x)), "box", ctx=other_ctx)
        refused(lambda: raw.spread(ball, values, base=foreign._map))
    got = dm.spread(ball, values, threshold, below).density
    assert_same_bits(got, checker.spread(x, ball, values, cases.intervals_of("box"), threshold, below), "after the refusals")
    assert gpu_ctx._lib.pdbeda_map_spread(*args()) == 0 and h.value          # the maximal table of one repeated offset is a legal call too
    _native.DeviceMap._made(raw, h)                                          # (owned and freed like any made map)


def test_most_offsets_all_duplicates(gpu_ctx):
    """16384 copies of one offset: legal, walked (duplicates are not row-compilable), and rank 0 wherever that offset leads to a seed."""
    dm, x, threshold, below = seeded(gpu_ctx, "box", "noise30")
    offsets = np.tile(np.array([[2, -1, 1]], dtype=np.int32), (cases.MAX_OFFSETS, 1))
    values = cases.values_of(len(offsets))
    out, ctr = dm.spread(offsets, values, threshold, below, counters=True)
    want = checker.spread(x, offsets[:1], values[[0, -1]], cases.intervals_of("box"), threshold, below)
    assert_same_bits(out.density, want, "duplicates")
    assert ctr["rows"] == 0 and set(np.unique(out.density)) == {0.0, float(cases.MAX_OFFSETS)}


# ---- the methods built on the call, against compositions of the checker ----------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["box", "skew", "thin"])
def test_morphology_against_the_checker(gpu_ctx, geometry):
    """dilated, eroded (the complement of the dilated complement, which wraps more than once on `thin`), opened, closed, distanceFrom, softMask and
    maskedBy as what the checker gives for the table and the values each is documented to use."""
    from pdb_eda_amd import ccp4
    dm, x, threshold, _ = seeded(gpu_ctx, geometry, "blobs")
    h, iv = cases.header_of(geometry), cases.intervals_of(geometry)
    ball, distance = ccp4.spreadTable(h, 1.0)
    n = len(ball)
    ones, zeros = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    dil = checker.spread(x, ball, np.append(ones, 0), iv, threshold)
    ero = checker.spread(x, ball, np.append(zeros, 1), iv, threshold, below=True)
    assert 0.05 < dil.mean() < 0.95 and 0.02 < ero.mean() < dil.mean()
    assert_same_bits(dm.dilated(1.0, threshold).density, dil, "dilated")
    assert_same_bits(dm.eroded(1.0, threshold).density, ero, "eroded")
    assert_same_bits(dm.opened(1.0, threshold).density, checker.spread(ero, ball, np.append(ones, 0), iv, 0.5), "opened")
    assert_same_bits(dm.closed(1.0, threshold).density, checker.spread(dil, ball, np.append(zeros, 1), iv, 0.5, below=True), "closed")
    wide, wide_d = ccp4.spreadTable(h, 2.0)
    dist = dm.distanceFrom(2.0, threshold, beyond=99.0).density
    assert_same_bits(dist, checker.spread(x, wide, np.append(wide_d.astype(np.float32), np.float32(99.0)), iv, threshold), "distanceFrom")
    assert set(np.unique(dist)) >= {0.0, 0.5} and np.array_equal(dist == 0.0, checker.seeds_of(x, threshold))
    soft_values = ccp4.softEdgeValues(wide_d, 0.5, 1.5)
    soft = checker.spread(x, wide, soft_values, iv, threshold)
    assert_same_bits(dm.softMask(0.5, 1.5, threshold).density, soft, "softMask")
    assert len(np.unique(soft)) > 3
    base_grid = cases.base_of(geometry)
    base = device_map(gpu_ctx, geometry, base_grid, "base")
    assert_same_bits(base.maskedBy(dm, 0.5, 1.5, threshold).density, checker.spread(x, wide, soft_values, iv, threshold, base=base_grid), "maskedBy", nan_as_nan=True)


def test_erosion_wraps_on_thin(gpu_ctx):
    """A slab of 13 voxels along c that fills r and the 3-voxel periodic axis s: eroded by 2.5 A (5 voxels, more than s is long, so the reach
    wraps round it more than once and meets nothing but the slab) 5 voxels go from each end along c and 3 stay."""
    x = np.zeros(cases.shape_of("thin"), dtype=np.float32)
    x[:, :, 4:17] = 1.0
    dm = device_map(gpu_ctx, "thin", x, "slab")
    got = dm.eroded(2.5).density
    want = np.zeros_like(x)
    want[:, :, 9:12] = 1.0
    assert_same_bits(got, want, "eroded slab")
    ball = cases.table("ball25", "thin")[0]
    assert_same_bits(got, checker.spread(x, ball, np.append(np.zeros(len(ball), dtype=np.float32), np.float32(1)), cases.intervals_of("thin"), 0.5, below=True), "against the checker")


def _sphere_count(header, shape, xyz, radii):
    """How many spheres cover each stored voxel, in numpy: the voxel's coordinates from crs2xyz_array, float64 distances against float32 radii."""
    ns, nr, nc = shape
    crs = np.stack(np.meshgrid(np.arange(nc), np.arange(nr), np.arange(ns), indexing="ij"), axis=-1).reshape(-1, 3)
    pos = header.crs2xyz_array(crs.astype(np.float64))
    d2 = ((pos[:, None, :] - np.asarray(xyz, dtype=np.float64)[None, :, :]) ** 2).sum(axis=2)
    r = np.asarray(radii, dtype=np.float32).astype(np.float64)
    count = (d2 <= (r * r)[None, :]).sum(axis=1)
    margin = np.abs(np.sqrt(d2) - r[None, :]).min()
    out = np.zeros(shape, dtype=np.int64)
    out[crs[:, 2], crs[:, 1], crs[:, 0]] = count
    return out, margin


def test_atom_and_solvent_masks_on_skew(gpu_ctx):
    """atomMask against a numpy sphere test on the skewed cut-out (no voxel within 1e-6 A of a sphere, so no decision hinges on an ulp), and
    solventMask as the checker's spread of the complement of the grown mask."""
    from pdb_eda_amd import ccp4
    xyz, radii = cases.atoms("skew")
    h, shape, iv = cases.header_of("skew"), cases.shape_of("skew"), cases.intervals_of("skew")
    dm = device_map(gpu_ctx, "skew", np.zeros(shape, dtype=np.float32), "zeros")
    count, margin = _sphere_count(h, shape, xyz, radii)
    assert margin > 1e-6
    want = (count > 0).astype(np.float32)
    assert 0.05 < want.mean() < 0.95
    assert_same_bits(dm.atomMask(xyz, radii).density, want, "atomMask")
    probe, shrink = 0.6, 0.5
    grown_r = (radii.astype(np.float64) + probe).astype(np.float32)
    grown, margin = _sphere_count(h, shape, xyz, grown_r)
    assert margin > 1e-6
    grown = (grown > 0).astype(np.float32)
    ball = ccp4.spreadTable(h, shrink)[0]
    assert len(ball) > 1
    solvent = checker.spread(grown, ball, np.append(np.ones(len(ball), dtype=np.float32), np.float32(0)), iv, 0.5, below=True)
    got = dm.solventMask(xyz, radii, probe=probe, shrink=shrink).density
    assert_same_bits(got, solvent, "solventMask")
    assert 0.05 < solvent.mean() < 0.95 and (solvent >= 1.0 - grown).all() and (solvent != 1.0 - grown).any()
    n, mean, std = dm.atomMask(xyz, radii).maskStats(dm.solventMask(xyz, radii, probe=probe, shrink=shrink))
    assert n > 0 and mean >= 0.0 and std >= 0.0
