"""pdbeda_map_filter and pdbeda_map_local_stats on the MI355X path against tests/filter_checker.py, the plain numpy restatement of the
contracts in include/pdbeda.h -- TO THE BIT: the library is built with -ffp-contract=off, every sum has a fixed order and a lane owns its
output, so the float32 maps are compared as uint32 (where the checker has a NaN only the NaN-ness is compared).
tests/test_filter_host.py holds the checker itself against scipy."""
import ctypes
import io
import os

import numpy as np
import pytest

from conftest import load_analysis_case
import filter_cases
import filter_checker

pytestmark = pytest.mark.gpu

_maps, _wanted = {}, {}
TAPS = filter_cases.tap_sets()


def device_map(name, gpu_ctx, grid=None, tag="a"):
    """A DensityMatrix on the geometry ``name`` holding ``grid`` (default: the seeded map of that geometry)."""
    from pdb_eda_amd import ccp4, synthetic
    key = (name, tag)
    if key not in _maps:
        data = filter_cases.grid_of(name) if grid is None else grid
        _maps[key] = (ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(filter_cases.spec_of(name), data)), name, ctx=gpu_ctx), np.array(data, dtype=np.float32))
    return _maps[key]


def second_map(name, gpu_ctx):
    return device_map(name, gpu_ctx, filter_cases.grid_of(name, seed=1, offset=-0.5), tag="b")


def wanted(key, make):
    """The checker's answer, computed once per case and shared (never modified)."""
    if key not in _wanted:
        _wanted[key] = make()
    return _wanted[key]


def assert_same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    if differ.any():
        at = tuple(int(v[0]) for v in np.nonzero(differ))
        print("%s: %d of %d voxels differ, first at [s][r][c] = %s: got %r, want %r" % (what, int(differ.sum()), got.size, at, float(got[at]), float(want[at])))
    assert not differ.any(), what


def run_filter(gpu_ctx, name, taps, renormalize=False):
    dm, grid = device_map(name, gpu_ctx)
    t = TAPS[taps]
    want = wanted(("filter", name, taps, renormalize), lambda: filter_checker.map_filter(grid, t, filter_cases.intervals_of(name), renormalize))
    out = dm.filtered(t[0], t[1], t[2], renormalize)
    got = out.density
    assert list(out.header.ncrs) == list(dm.header.ncrs)
    assert_same_bits(got, want, "%s / %s%s" % (name, taps, " renormalised" if renormalize else ""))
    return got, want


@pytest.mark.parametrize("name", ["box", "skew", "rep", "unit", "past", "lanes", "lanes_past"])
@pytest.mark.parametrize("taps", ["gauss", "asym", "signed"])
def test_filter_against_checker(gpu_ctx, name, taps):
    """A periodic box, a cut-out with permuted axes, a start and three intervals, a stored box larger than its cell, exactly one work unit
    of every pass and one voxel past it; three different Gaussian radii, asymmetric taps (a reversed window shows), taps of both signs."""
    got, want = run_filter(gpu_ctx, name, taps)
    assert np.isfinite(got).all() and float(np.abs(got).max()) > 0.1          # (a vacuous comparison cannot pass)


def test_work_units_are_the_kernels():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pdb_eda_amd", "csrc", "pdbeda_filter.h")).read()
    for name, value in (("FC_RUN", filter_cases.UNIT_C[0]), ("FC_ROWS", filter_cases.UNIT_C[1]), ("FL_LANES", filter_cases.UNIT_LINE[0]), ("FL_CHUNK", filter_cases.UNIT_LINE[1])):
        assert "constexpr int %s = %d;" % (name, value) in text


def test_identity_taps(gpu_ctx):
    """Radius 0 with [1.0] on all axes: the map itself, except that -0.0 becomes +0.0 (the sum starts at +0.0)."""
    grid = np.array(filter_cases.grid_of("box"))
    grid[0, 0, :4] = [-0.0, 0.0, -1.0, 1e-30]
    dm, _ = device_map("box", gpu_ctx, grid, tag="zeros")
    got = dm.filtered(np.ones(1), np.ones(1), np.ones(1)).density
    want = grid.copy()
    want[0, 0, 0] = 0.0
    assert_same_bits(got, want, "identity")
    assert_same_bits(got, filter_checker.map_filter(grid, TAPS["identity"], filter_cases.intervals_of("box")), "identity against the checker")


def test_radius_wraps_the_axis_more_than_once(gpu_ctx):
    """Radius 24 on the 21-voxel periodic axis; the same radius on the cut-out and the repeating box."""
    for name in ("box", "skew", "rep"):
        run_filter(gpu_ctx, name, "wrap24")


@pytest.mark.parametrize("name", ["line", "cut"])
def test_largest_radius(gpu_ctx, name):
    """Radius 64 along a 70-voxel line, periodic and as a cut-out of a 100-step cell, with and without renormalisation."""
    run_filter(gpu_ctx, name, "r64")
    got, want = run_filter(gpu_ctx, name, "r64", renormalize=True)
    assert (got > 0).all()


@pytest.mark.parametrize("taps", ["gauss", "asym", "box", "one_sided"])
def test_renormalised_on_a_cut_out(gpu_ctx, taps):
    """skew: a box window leaves N = 0 nowhere; taps with zeros at one end do, at the high faces, and those voxels are exactly +0.0f."""
    plain, _ = run_filter(gpu_ctx, "skew", taps)
    got, want = run_filter(gpu_ctx, "skew", taps, renormalize=True)
    n = filter_checker.norm3(got.shape, TAPS[taps], filter_cases.intervals_of("skew"))
    if taps == "one_sided":
        assert (n == 0).any() and np.all(got[n == 0].view(np.uint32) == 0)
    else:
        assert (n > 0).all()
    assert not np.array_equal(plain, got)


def run_stats(gpu_ctx, name, taps, pair, std_floor, a=None, b=None, tag=None):
    dm, ga = a if a is not None else device_map(name, gpu_ctx)
    other, gb = (b if b is not None else second_map(name, gpu_ctx)) if pair else (None, None)
    t = TAPS[taps]
    want = wanted(("stats", name, taps, pair, std_floor, tag), lambda: filter_checker.local_stats(ga, gb, t, filter_cases.intervals_of(name), std_floor))
    made = dm._map.local_stats(other._map if pair else None, t[0], t[1], t[2], std_floor)
    assert sorted(made) == sorted(want)
    got = dict((key, dm._made(m).density) for key, m in made.items())
    for key in sorted(want):
        assert_same_bits(got[key], want[key], "%s / %s / %s%s: %s" % (name, taps, "pair" if pair else "one", " / floor %g" % std_floor if std_floor else "", key))
    return dm, other, got, want


@pytest.mark.parametrize("name", ["box", "skew"])
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("std_floor", [0.0, 0.4])
def test_local_stats_against_checker(gpu_ctx, name, pair, std_floor):
    dm, other, got, want = run_stats(gpu_ctx, name, "gauss", pair, std_floor)
    assert float(got["std_a"].min()) > 0 and float(np.abs(got["z_a"]).max()) > 0.5 and 1.0 < float(got["mean_a"].mean()) < 2.0
    if std_floor:
        assert (want["std_a"] < std_floor).any() and (want["std_a"] > std_floor).any()          # (both sides of the floor)
    if pair:
        assert float(got["cc"].min()) >= -1.0 and float(got["cc"].max()) <= 1.0 and float(np.abs(got["cc"]).max()) > 0.2


@pytest.mark.parametrize("taps", ["box", "one_sided", "asym"])
def test_local_stats_other_windows(gpu_ctx, taps):
    """On the cut-out: a box window, an asymmetric one, and one that leaves N = 0 at the high faces (every output exactly 0 there)."""
    dm, other, got, want = run_stats(gpu_ctx, "skew", taps, True, 0.0)
    n = filter_checker.norm3(got["cc"].shape, TAPS[taps], filter_cases.intervals_of("skew"))
    if taps == "one_sided":
        assert (n == 0).any() and all(np.all(v[n == 0].view(np.uint32) == 0) for v in got.values())


def test_local_stats_of_a_constant_map(gpu_ctx):
    const = np.full(filter_cases.grid_of("skew").shape, 3.0, dtype=np.float32)
    a = device_map("skew", gpu_ctx, const, tag="const")
    dm, other, got, want = run_stats(gpu_ctx, "skew", "box", True, 0.0, a=a, tag="const")
    zero_var = want["std_a"] == 0
    assert zero_var.any() and np.all(got["z_a"][zero_var] == 0) and np.all(got["cc"][zero_var] == 0)
    run_stats(gpu_ctx, "skew", "box", False, 0.5, a=a, tag="const")


def test_local_stats_of_a_linear_pair(gpu_ctx):
    """b = 2 a + 1 (exact in float32 for these values rounded to 12 bits): cc = 1 after clamping wherever both variances are positive."""
    ga = (np.round(filter_cases.grid_of("box").astype(np.float64) * 256.0) / 256.0).astype(np.float32)
    gb = (2.0 * ga.astype(np.float64) + 1.0).astype(np.float32)
    assert np.array_equal(gb.astype(np.float64), 2.0 * ga.astype(np.float64) + 1.0)
    a, b = device_map("box", gpu_ctx, ga, tag="lin-a"), device_map("box", gpu_ctx, gb, tag="lin-b")
    dm, other, got, want = run_stats(gpu_ctx, "box", "gauss", True, 0.0, a=a, b=b, tag="lin")
    assert (got["std_a"] > 0).all() and np.all(np.abs(got["cc"] - 1.0) <= 1e-6) and float(got["cc"].max()) <= 1.0


def test_outputs_one_at_a_time_equal_those_together(gpu_ctx):
    from pdb_eda_amd import _native
    dm, other, got, want = run_stats(gpu_ctx, "skew", "gauss", True, 0.4)
    t = TAPS["gauss"]
    for key in _native.LOCAL_STATS_OUTPUTS:
        made = dm._map.local_stats(other._map, t[0], t[1], t[2], 0.4, want=(key,))
        assert list(made) == [key]
        assert dm._made(made[key]).density.tobytes() == got[key].tobytes(), key
    alone = dm._map.local_stats(None, t[0], t[1], t[2], 0.4)
    for key in ("mean_a", "std_a", "z_a"):                      # (the channels of a do not depend on b being there)
        assert dm._made(alone[key]).density.tobytes() == got[key].tobytes(), key


def test_one_infinite_voxel_spreads_as_in_the_checker(gpu_ctx):
    grid = np.array(filter_cases.grid_of("skew"))
    grid[3, 4, 10] = np.inf
    with np.errstate(invalid="ignore"):                         # (the header's own statistics of a map with an infinity)
        dm, _ = device_map("skew", gpu_ctx, grid, tag="inf")
    for taps in ("gauss", "signed", "one_sided"):               # (one_sided: 0 * inf inside the window is a NaN)
        t = TAPS[taps]
        want = filter_checker.map_filter(grid, t, filter_cases.intervals_of("skew"))
        got = dm.filtered(t[0], t[1], t[2]).density
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), taps
        assert_same_bits(got, want, "inf / " + taps)
        assert (~np.isfinite(want)).any() and np.isfinite(want).any()
    assert np.isnan(filter_checker.map_filter(grid, TAPS["one_sided"], filter_cases.intervals_of("skew"))).any()


def test_two_runs_give_identical_bytes(gpu_ctx):
    dm, _ = device_map("past", gpu_ctx)
    other, _ = second_map("past", gpu_ctx)
    t = TAPS["asym"]
    assert dm.filtered(t[0], t[1], t[2], True).density.tobytes() == dm.filtered(t[0], t[1], t[2], True).density.tobytes()
    first = dm._map.local_stats(other._map, t[0], t[1], t[2], 0.1)
    again = dm._map.local_stats(other._map, t[0], t[1], t[2], 0.1)
    for key in first:
        assert dm._made(first[key]).density.tobytes() == dm._made(again[key]).density.tobytes(), key


# ---- refusals: PDBEDA_ERR_ARGUMENT, the out pointers untouched, the context usable -------------------------------------------------------
SENTINEL = 0x5A5A5A5A


def _raw_filter(dm, taps, radii, flags):
    lib = dm._ctx._lib
    out = ctypes.c_void_p(SENTINEL)
    arrays = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in taps]
    ptrs = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
    rc = lib.pdbeda_map_filter(dm._map._h, ptrs[0], radii[0], ptrs[1], radii[1], ptrs[2], radii[2], flags, ctypes.byref(out))
    return rc, out.value


def _raw_stats(dm, other, taps, radii, std_floor, want):
    from pdb_eda_amd import _native
    lib = dm._ctx._lib
    outs = dict((key, ctypes.c_void_p(SENTINEL)) for key in want)
    arrays = [np.ascontiguousarray(t, dtype=np.float64) for t in taps]
    refs = [ctypes.byref(outs[key]) if key in outs else None for key in _native.LOCAL_STATS_OUTPUTS]
    rc = lib.pdbeda_map_local_stats(dm._map._h, None if other is None else other._map._h, arrays[0].ctypes.data_as(ctypes.c_void_p), radii[0],
                                    arrays[1].ctypes.data_as(ctypes.c_void_p), radii[1], arrays[2].ctypes.data_as(ctypes.c_void_p), radii[2], ctypes.c_double(std_floor), *refs)
    return rc, [v.value for v in outs.values()]


def test_refusals(gpu_ctx):
    from pdb_eda_amd import _native
    dm, grid = device_map("box", gpu_ctx)
    other, _ = second_map("box", gpu_ctx)
    small, _ = device_map("lanes", gpu_ctx)                     # (another shape: skew and rep have box's ncrs)
    one, big = np.ones(1), np.full(2 * 65 + 1, 1.0 / 131)
    nan_tap, neg_tap = np.array([0.25, np.nan, 0.25]), np.array([0.5, -0.25, 0.75])
    good = TAPS["gauss"]

    def good_call_follows():
        assert_same_bits(dm.filtered(good[0], good[1], good[2]).density, wanted(("filter", "box", "gauss", False), lambda: filter_checker.map_filter(grid, good, filter_cases.intervals_of("box"))),
                         "a good call after a refusal")

    filters = [
        ("radius 65", (big, one, one), (65, 0, 0), 0),
        ("radius -1", (one, one, one), (0, -1, 0), 0),
        ("a NaN tap", (one, one, nan_tap), (0, 0, 1), 0),
        ("an infinite tap", (np.array([np.inf]), one, one), (0, 0, 0), 0),
        ("a NULL tap", (one, None, one), (0, 0, 0), 0),
        ("a negative tap under renormalisation", (one, neg_tap, one), (0, 1, 0), _native.FILTER_RENORMALIZE),
        ("an unknown flag", (one, one, one), (0, 0, 0), 2),
    ]
    for what, taps, radii, flags in filters:
        rc, out = _raw_filter(dm, taps, radii, flags)
        assert rc == _native.PDBEDA_ERR_ARGUMENT and out == SENTINEL, what
        good_call_follows()
    rc, out = _raw_filter(dm, (one, neg_tap, one), (0, 1, 0), 0)          # (allowed without the flag)
    assert rc == 0 and out not in (None, SENTINEL)
    assert dm._ctx._lib.pdbeda_map_free(ctypes.c_void_p(out)) == 0

    all_a, all_b = ("mean_a", "std_a", "z_a"), _native.LOCAL_STATS_OUTPUTS
    stats = [
        ("a NaN std_floor", other, (one, one, one), (0, 0, 0), float("nan"), all_b),
        ("a negative std_floor", other, (one, one, one), (0, 0, 0), -0.5, all_b),
        ("cc without b", None, (one, one, one), (0, 0, 0), 0.0, ("mean_a", "cc")),
        ("mean_b without b", None, (one, one, one), (0, 0, 0), 0.0, ("mean_b",)),
        ("maps of two shapes", small, (one, one, one), (0, 0, 0), 0.0, all_b),
        ("a negative tap", other, (one, neg_tap, one), (0, 1, 0), 0.0, all_b),
        ("radius 65", None, (big, one, one), (65, 0, 0), 0.0, all_a),
        ("a NaN tap", None, (one, one, nan_tap), (0, 0, 1), 0.0, all_a),
    ]
    for what, b, taps, radii, floor, want in stats:
        rc, outs = _raw_stats(dm, b, taps, radii, floor, want)
        assert rc == _native.PDBEDA_ERR_ARGUMENT and all(v == SENTINEL for v in outs), what
        good_call_follows()
    with pytest.raises(_native.PdbedaError) as info:
        dm.filtered(big, one, one)
    assert info.value.code == _native.PDBEDA_ERR_ARGUMENT and "65" in str(info.value)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_gaussian_filter_in_angstrom(gpu_ctx):
    from pdb_eda_amd import ccp4
    dm, grid = device_map("box", gpu_ctx)                       # 0.5 A steps: 0.75 A = 1.5 steps
    t = ccp4.gaussianTaps(1.5)
    got = dm.gaussianFilter(0.75, renormalize=False).density
    assert got.tobytes() == dm.filtered(t, t, t).density.tobytes()
    assert got.tobytes() == dm.gaussianFilter(1.5, voxels=True, renormalize=False).density.tobytes()
    assert_same_bits(dm.gaussianFilter(0.75).density, filter_checker.map_filter(grid, (t, t, t), filter_cases.intervals_of("box"), True), "gaussianFilter, renormalised")
    stats = dm.localStats(second_map("box", gpu_ctx)[0], sigma=0.75, stdFloor=0.1)
    assert sorted(stats) == ["cc", "mean", "meanOther", "std", "stdOther", "z"]
    want = filter_checker.local_stats(grid, filter_cases.grid_of("box", seed=1, offset=-0.5), (t, t, t), filter_cases.intervals_of("box"), 0.1)
    assert_same_bits(stats["z"].density, want["z_a"], "localStats z")
    assert_same_bits(stats["cc"].density, want["cc"], "localStats cc")
    one = dm.localStats(taps=ccp4.boxTaps(1))
    assert sorted(one) == ["mean", "std", "z"]
    b = ccp4.boxTaps(1)
    assert_same_bits(one["mean"].density, filter_checker.local_stats(grid, None, (b, b, b), filter_cases.intervals_of("box"))["mean_a"], "localStats of box taps")


@pytest.fixture(scope="module")
def analyzer(gpu_ctx):
    """The small analysis golden entry, as tests/test_gpu_model.py sets it up."""
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    st.header = {"resolution": 2.0}
    return densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb)


def test_local_z_map_can_be_labelled(analyzer):
    from pdb_eda_amd import densityAnalysis
    stats = analyzer.localDiffStats
    assert sorted(stats) == ["mean", "std", "z"]
    zmap = analyzer.localZDiffObj
    grid, diff = zmap.density, analyzer.diffDensityObj
    assert np.isfinite(grid).all() and list(zmap.header.ncrs) == list(diff.header.ncrs)
    taps = analyzer._localTaps(diff)
    want = filter_checker.local_stats(diff.density, None, taps, [int(v) for v in diff.header.crsInterval], densityAnalysis.localStdFloorFraction * diff.stdDensity)
    assert_same_bits(grid, want["z_a"], "the entry's local z map")
    green, red = analyzer.localGreenBlobList, analyzer.localRedBlobList
    u = zmap.header.uniqueNcrs
    box = grid[:u[2], :u[1], :u[0]]
    print("local z: min %.3f max %.3f; %d green / %d red local blobs, %d / %d global" % (float(grid.min()), float(grid.max()), len(green), len(red), len(analyzer.greenBlobList),
                                                                                      len(analyzer.redBlobList)))
    assert sum(b.numVoxels for b in green) == int((box >= 3.0).sum()) and sum(b.numVoxels for b in red) == int((box <= -3.0).sum())
    assert all(b.totalDensity > 0 for b in green) and all(b.totalDensity < 0 for b in red)
    cc = analyzer.localModelCorrelationObj.density
    assert np.isfinite(cc).all() and -1.0 <= float(cc.min()) and float(cc.max()) <= 1.0 and float(cc.max()) > 0.3


def test_atom_local_table(analyzer):
    rows = analyzer.calculateAtomLocalCorrelations()
    model_rows = analyzer.calculateAtomModelCorrelations()
    assert analyzer.atomLocalHeader == ["model", "chain", "residue_number", "residue_name", "atom_name", "occupancy", "bfactor", "local_cc", "local_z_diff", "local_std_diff"]
    assert len(rows) == len(model_rows) > 0 and all(len(r) == 10 for r in rows)
    assert [list(r[:7]) for r in rows] == [list(r[:7]) for r in model_rows]
    values = np.array([r[7:] for r in rows], dtype=np.float64)
    assert np.isfinite(values).all() and np.all(np.abs(values[:, 0]) <= 1.0) and np.all(values[:, 2] >= 0)
    residues = analyzer.calculateResidueLocalCorrelations()
    assert 0 < len(residues) <= len(rows) and all(len(r) == len(analyzer.residueLocalHeader) for r in residues) and all(r[5] >= r[6] for r in residues)      # (mean >= minimum)
    summary = analyzer.localSummary()
    assert summary["num_local_green_blobs"] == len(analyzer.localGreenBlobList) and summary["min_atom_local_cc"] <= summary["median_atom_local_cc"]
    assert summary["min_atom_local_cc"] == float(values[:, 0].min()) and summary["radius_c"] == len(analyzer._localTaps(analyzer.diffDensityObj)[0]) // 2


def test_single_structure_local_mode(analyzer, tmp_path):
    from pdb_eda_amd import singleStructure
    counts = {"atom": len(analyzer.calculateAtomModelCorrelations()), "residue": len(analyzer.calculateResidueModelCorrelations()), "summary": 1}
    for level in ("atom", "residue", "summary"):
        header, rows = singleStructure.rows(analyzer, "local", level)
        assert len(rows) == counts[level] and all(len(r) == len(header) for r in rows), level
        path = tmp_path / ("local_%s.csv" % level)
        singleStructure.write(header, rows, str(path), "csv")
        lines = path.read_text().strip().splitlines()
        assert len(lines) == len(rows) + 1 and lines[0] == ",".join(header), level
    with pytest.raises(ValueError):
        singleStructure.rows(analyzer, "local", "domain")
