"""pdbeda_map_resample on the MI355X path against tests/resample_checker.py, the plain numpy restatement of the contract in
include/pdbeda.h -- TO THE BIT: the library is built with -ffp-contract=off, the operators are taken in index order and a lane owns its
voxel, so the float32 maps are compared as uint32 (where the checker has a NaN only the NaN-ness is compared).
tests/test_resample_host.py holds the checker itself against scipy, and guards every case here against being vacuous."""
import ctypes
import io
import os

import numpy as np
import pytest

import resample_cases as rc
import resample_checker as chk

pytestmark = pytest.mark.gpu

_maps = {}
STAGE_SWITCH = "PDBEDA_RESAMPLE_STAGE"


def matrix_on(header, grid, gpu_ctx, tag):
    from pdb_eda_amd import ccp4
    return ccp4.DensityMatrix(header, header.origin, np.array(grid, dtype=np.float32), tag, ctx=gpu_ctx)


def source(name, gpu_ctx):
    """The seeded map of the geometry ``name`` as a resident DensityMatrix (made once)."""
    if name not in _maps:
        _maps[name] = matrix_on(rc.header_of(name), rc.grid_of(name), gpu_ctx, name)
    return _maps[name]


def assert_same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    if differ.any():
        at = tuple(int(v[0]) for v in np.nonzero(differ))
        print("%s: %d of %d voxels differ, first at [s][r][c] = %s: got %r, want %r" % (what, int(differ.sum()), got.size, at, float(got[at]), float(want[at])))
    assert not differ.any(), what


def run_case(gpu_ctx, name, order, coverage=False, stage=None):
    """The device's answer to a case: (out, coverage or None, counters).  ``stage``: the value of the staging switch for this call."""
    case = rc.cases()[name]
    src = source(case["src"], gpu_ctx)
    base = matrix_on(case["dst"], case["base"], gpu_ctx, "base") if "base" in case else None
    before = os.environ.get(STAGE_SWITCH)
    try:
        if stage is not None:
            os.environ[STAGE_SWITCH] = stage
        made = src.resampled(case["dst"], case["ops"], order=order, mean=case["mean"], fill=case["fill"], base=base, alpha=case.get("alpha", 1.0), coverage=coverage)
    finally:
        if stage is not None:
            if before is None:
                del os.environ[STAGE_SWITCH]
            else:
                os.environ[STAGE_SWITCH] = before
    out, cover = made if coverage else (made, None)
    assert list(out.header.ncrs) == list(case["dst"].ncrs)
    return out.density, (cover.density if coverage else None), out.resampleCounters


def test_tile_constants_are_the_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "pdb_eda_amd", "csrc", "pdbeda_resample.h")).read()
    assert "constexpr int RS_C = %d, RS_R = %d, RS_S = %d;" % rc.TILE in text
    assert "constexpr int RS_LDS_VOX = %d;" % rc.LDS_VOX in text
    assert "#define PDBEDA_RESAMPLE_MAX_OPS %d\n" % rc.MAX_OPS in open(os.path.join(root, "include", "pdbeda.h")).read()


@pytest.mark.parametrize("order", rc.ORDERS)
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_bits_against_checker(gpu_ctx, name, order):
    """Every case of tests/resample_cases.py: the three source geometries under a general rotation plus shift, a finer and a coarser
    destination, one tile and one voxel past it, first-valid and mean mode on a cut-out with a NaN, a -0.0 and a plain fill, one, two and
    192 operators, base + alpha * value, and the two destinations on either side of the LDS budget -- the map, its coverage and the two
    voxel counters."""
    want, count = rc.wanted(name, order)
    got, cover, counters = run_case(gpu_ctx, name, order, coverage=True)
    assert_same_bits(got, want, "%s at order %d" % (name, order))
    assert np.array_equal(cover, count.astype(np.float32)), "coverage of %s at order %d" % (name, order)
    assert counters["covered"] == int((count > 0).sum()) and counters["uncovered"] == int((count == 0).sum())
    fill = np.asarray(rc.cases()[name]["fill"], dtype=np.float32).reshape(1)
    if (count == 0).any() and not np.isnan(fill[0]):
        assert set(got.view(np.uint32)[count == 0].tolist()) == {int(fill.view(np.uint32)[0])}          # the fill's bits: -0.0 stays -0.0


def test_second_operator_serves_what_the_first_cannot(gpu_ctx):
    case = rc.cases()["cutout-nan"]
    header, grid = rc.header_of(case["src"]), rc.grid_of(case["src"])
    _, first = chk.resample(header, grid, case["dst"], case["ops"][:1], 1)
    _, both = rc.wanted("cutout-nan", 1)
    gained = int(((both > 0) & (first == 0)).sum())
    assert gained > 100                                                   # (the case is what it says, by the checker)
    got, _, counters = run_case(gpu_ctx, "cutout-nan", 1)
    assert counters["covered"] == int((first > 0).sum()) + gained and int(np.isnan(got).sum()) == counters["uncovered"]


@pytest.mark.parametrize("order", rc.ORDERS)
@pytest.mark.parametrize("name", rc.SOURCES)
def test_identity_returns_the_map(gpu_ctx, name, order):
    src = source(name, gpu_ctx)
    out = src.resampled(src.header, order=order, fill=np.nan)
    assert out.density.tobytes() == rc.grid_of(name).tobytes() and out.resampleCounters["uncovered"] == 0


@pytest.mark.parametrize("order", rc.ORDERS)
def test_whole_grid_steps_roll_the_map(gpu_ctx, order):
    src = source("box", gpu_ctx)
    out = src.resampled(src.header, rc.grid_shift(src.header, (5, -2, 3)), order=order)
    assert out.density.tobytes() == np.roll(rc.grid_of("box"), (-3, 2, -5), axis=(0, 1, 2)).tobytes()


@pytest.mark.parametrize("order", rc.ORDERS)
def test_two_fold_flips_the_map(gpu_ctx, order):
    src = source("box", gpu_ctx)
    out = src.resampled(src.header, np.hstack([np.diag([-1.0, -1.0, 1.0]), np.zeros((3, 1))]), order=order)
    assert out.density.tobytes() == np.roll(rc.grid_of("box")[:, ::-1, ::-1], (1, 1), axis=(1, 2)).tobytes()


def test_base_is_combine_of_a_resampled_map(gpu_ctx):
    """Everything covered.  At order 0 a value is a voxel, float32(value) loses nothing, and base + alpha * value in one call equals
    pdbeda_map_combine of the base with the separately resampled map to the bit.  At order 1 the two-call route rounds the value to
    float32 in between: it equals ITS restatement, float32(base + alpha * float32(value)), and lies within one float32 spacing of the one call."""
    from pdb_eda_amd import _native, ccp4
    case = rc.cases()["base-box"]
    src = source("box", gpu_ctx)
    base = matrix_on(case["dst"], case["base"], gpu_ctx, "base")

    def two_calls(order):
        plain = src.resampled(case["dst"], case["ops"], order=order)
        assert plain.resampleCounters["uncovered"] == 0
        return ccp4.DensityMatrix.fromDeviceMap(case["dst"], case["dst"].origin, _native.DeviceMap.combine(base._map, plain._map, case["alpha"]), "two", gpu_ctx).density

    assert run_case(gpu_ctx, "base-box", 0)[0].tobytes() == two_calls(0).tobytes()
    value32 = chk.resample(rc.header_of("box"), rc.grid_of("box"), case["dst"], case["ops"], 1)[0]
    want = (case["base"].astype(np.float64) + case["alpha"] * value32.astype(np.float64)).astype(np.float32)
    got = two_calls(1)
    assert_same_bits(got, want, "combine of a resampled map")
    one_call = run_case(gpu_ctx, "base-box", 1)[0]
    assert float(np.abs(one_call.astype(np.float64) - got.astype(np.float64)).max()) <= 2.0 ** -22 * float(np.abs(one_call).max())


@pytest.mark.parametrize("order", rc.ORDERS)
@pytest.mark.parametrize("name", ["rotated-skew", "finer", "coarser", "cutout-nan", "cutout-mean", "mean-2", "base-cutout", "budget-inside", "budget-outside"])
def test_staging_changes_no_bit(gpu_ctx, name, order):
    """Staged boxes, direct loads only, and staged boxes that are NOT grown -- so that the lanes at a tile's rim leave them and read the map
    directly for that sample --: one result.  The counters say which path ran: per (tile, operator) the box the kernel stages is restated
    in tests/resample_cases.py, and a pair is staged iff the order is 3 and that box holds at most RS_LDS_VOX voxels."""
    case = rc.cases()[name]
    on, _, ctr_on = run_case(gpu_ctx, name, order, stage="1")
    off, _, ctr_off = run_case(gpu_ctx, name, order, stage="0")
    tight, _, ctr_tight = run_case(gpu_ctx, name, order, stage="2")
    assert on.tobytes() == off.tobytes() and on.tobytes() == tight.tobytes()
    assert_same_bits(on, rc.wanted(name, order)[0], "%s at order %d, staged" % (name, order))
    boxes = rc.tile_footprints(case, order)
    assert ctr_off["stagedPairs"] == 0
    if case["mean"] or len(case["ops"]) == 1:          # (first-valid mode leaves the operator loop early: its pairs are bounded, not fixed)
        assert ctr_on["stagedPairs"] == rc.staged_pairs(case, order) and ctr_on["stagedPairs"] + ctr_on["directPairs"] == boxes.size
        assert ctr_off["directPairs"] == boxes.size
        assert ctr_tight["stagedPairs"] == rc.staged_pairs(case, order, grown=False)
    else:
        assert len(boxes) <= ctr_on["stagedPairs"] + ctr_on["directPairs"] <= boxes.size
    if order in rc.STAGED_ORDERS:
        assert (ctr_on["stagedPairs"] > 0) == (name != "coarser")               # (a tile of the coarser destination spans more source voxels than the budget)
        if name == "budget-inside":
            assert ctr_on["directPairs"] == 0
        if name == "budget-outside":
            assert ctr_on["directPairs"] > 0                                   # both paths in one launch
    else:
        assert ctr_on["stagedPairs"] == 0 and ctr_tight["stagedPairs"] == 0    # orders 0 and 1 never stage


def test_a_lane_leaves_the_ungrown_box():
    """By the restatement: in the ungrown box of ``finer``'s first tile some voxels' order-3 supports (b - 1 .. b + 2) end outside, others'
    do not -- the case test_staging_changes_no_bit runs with switch value 2 does hold lanes that take the direct path inside a staged pair."""
    case = rc.cases()["finer"]
    src, dst = rc.header_of(case["src"]), case["dst"]
    crs = chk.all_crs(dst)
    tile = crs[(crs[:, 0] < rc.TILE[0]) & (crs[:, 1] < rc.TILE[1]) & (crs[:, 2] < rc.TILE[2])]
    f = chk.snap(chk.xyz2frac(src, chk.apply_operator(case["ops"][0], chk.crs2xyz(dst, tile))))
    corners = np.array([[c, r, s] for c in (0, rc.TILE[0] - 1) for r in (0, rc.TILE[1] - 1) for s in (0, rc.TILE[2] - 1)])
    fc = chk.xyz2frac(src, chk.apply_operator(case["ops"][0], chk.crs2xyz(dst, corners)))
    lo, hi = np.floor(fc.min(axis=0)), np.ceil(fc.max(axis=0))
    outside = ((np.floor(f) - 1 < lo) | (np.floor(f) + 2 > hi)).any(axis=1)
    assert outside.any() and not outside.all()


def test_two_calls_agree_to_the_bit(gpu_ctx):
    for name, order in (("mean-192", 3), ("cutout-nan", 1), ("finer", 3)):
        a, ca, _ = run_case(gpu_ctx, name, order, coverage=True)
        b, cb, _ = run_case(gpu_ctx, name, order, coverage=True)
        assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()


def raw_call(ctx, src_map, geometry, ops, n_ops, order, flags, base=None, alpha=1.0, want_coverage=True):
    """pdbeda_map_resample as the header declares it: (status, out handle, coverage handle, counters)."""
    out, cover = ctypes.c_void_p(), ctypes.c_void_p()
    counters = np.full(4, -1, dtype=np.int64)
    ops = np.ascontiguousarray(ops, dtype=np.float64)
    rc_ = ctx._lib.pdbeda_map_resample(src_map._h, ctypes.byref(geometry), ops.ctypes.data_as(ctypes.c_void_p), n_ops, order, flags, ctypes.c_float(0.0),
                                       base._h if base is not None else None, ctypes.c_double(alpha), ctypes.byref(out), ctypes.byref(cover) if want_coverage else None,
                                       counters.ctypes.data_as(ctypes.c_void_p))
    return rc_, out.value, cover.value, counters


def test_refusals_leave_everything_untouched(gpu_ctx):
    from pdb_eda_amd import _native
    src = source("box", gpu_ctx)
    dst = rc.cases()["rotated-box"]["dst"]
    good = rc.cases()["rotated-box"]["ops"]
    other_shape = matrix_on(rc.header_of("box"), rc.grid_of("box"), gpu_ctx, "other")
    second_ctx = _native.Context(gpu_ctx.device)
    try:
        elsewhere = _native.DeviceMap(second_ctx, np.zeros((dst.ncrs[2], dst.ncrs[1], dst.ncrs[0]), dtype=np.float32), dst.geometry())

        def geometry(**change):
            g = dst.geometry()
            for axis, n in change.items():
                g.ncrs["crs".index(axis)] = n
            return g

        bad_entry, far = good.copy(), good.copy()
        bad_entry[0, 5] = np.inf
        far[0, 3] = 1e9                                              # 2e9 grid steps of 0.5 A away
        nan_entry = good.copy()
        nan_entry[0, 11] = np.nan
        many = np.tile(good, (rc.MAX_OPS + 1, 1))
        refused = {
            "no operator": dict(ops=good, n_ops=0), "too many operators": dict(ops=many, n_ops=rc.MAX_OPS + 1), "order 2": dict(order=2), "order -1": dict(order=-1),
            "unknown flag": dict(flags=2), "infinite entry": dict(ops=bad_entry), "NaN entry": dict(ops=nan_entry), "infinite alpha": dict(alpha=np.inf),
            "NaN alpha": dict(alpha=np.nan), "base of another shape": dict(base=other_shape._map), "base of another context": dict(base=elsewhere),
            "empty axis": dict(geometry=geometry(r=0)), "axis of 2^30": dict(geometry=geometry(c=1 << 30)), "2^29 steps away": dict(ops=far),
        }
        for what, change in refused.items():
            args = dict(geometry=dst.geometry(), ops=good, n_ops=1, order=1, flags=0, base=None, alpha=1.0)
            args.update(change)
            status, out, cover, counters = raw_call(gpu_ctx, src._map, **args)
            assert status == _native.PDBEDA_ERR_ARGUMENT, what
            assert out is None and cover is None and (counters == -1).all(), what
            # the context is usable: the next call is served
            ok = src.resampled(dst, good, order=1)
            assert_same_bits(ok.density, rc.wanted("rotated-box", 1)[0], "after the refusal of %s" % what)
        # the largest list is not refused
        status, out, cover, _ = raw_call(gpu_ctx, src._map, dst.geometry(), many[:rc.MAX_OPS], rc.MAX_OPS, 0, 1)
        assert status == 0 and out and cover
        for handle in (out, cover):
            assert gpu_ctx._lib.pdbeda_map_free(ctypes.c_void_p(handle)) == 0
        del elsewhere
    finally:
        second_ctx.close()


# ---- the analysis layer: two entries of one molecule -------------------------------------------------------------------------------------
def _entry(gpu_ctx, name, header, grid, atoms, rotation_mats=None):
    from pdb_eda_amd import densityAnalysis, structure
    st = structure.Structure(name)
    chain = structure.Chain("A", structure.Model(0, st))
    for i, xyz in enumerate(atoms):
        structure.Atom("CA", xyz, 1.0, 20.0, "C", structure.Residue((" ", i + 1, " "), "ALA", chain), i + 1)
    pdb = structure.PDBEntry(structure.PDBHeader(pdbid=name, resolution=2.0, spaceGroup="P_1", rotationMats=rotation_mats))
    dens = matrix_on(header, grid, gpu_ctx, name)
    return densityAnalysis.DensityAnalysis(name, dens, matrix_on(header, np.zeros_like(grid), gpu_ctx, name), st, pdb)


@pytest.fixture(scope="module")
def pair(gpu_ctx):
    p = rc.entry_pair()
    return p, _entry(gpu_ctx, "first", *p["first"]), _entry(gpu_ctx, "second", *p["second"])


def test_operator_between_two_entries(pair):
    p, first, second = pair
    op, rmsd, n = first.operatorTo(second)
    assert n == len(p["first"][2]) and rmsd < 1e-4          # (atom coordinates are float32)
    assert float(np.abs(op - p["motion"]).max()) < 1e-4
    with pytest.raises(ValueError):
        first.operatorTo(second, atomName="CB")


def test_compare_maps_of_two_entries(pair):
    """cc against a bound from the checker: the checker resamples the second entry's grid onto the first's with the known motion, and numpy
    correlates it with the first over the covered voxels.  The device's map has the checker's bits, so its cc differs from that only by
    the order of the five sums: the bound is the checker's cc minus 1e-6 -- and the checker's own cc is above 0.95, the same molecule
    seen through trilinear interpolation, with two planted sites on one side."""
    p, first, second = pair
    (h1, g1, _), (h2, g2, _) = p["first"], p["second"]
    moved, count = chk.resample(h2, g2, h1, p["motion"], 1, fill=np.nan)
    covered = count > 0
    a, b = g1[covered].astype(np.float64), moved[covered].astype(np.float64)
    cc_checker = float(np.corrcoef(a, b)[0, 1])
    scale_checker = float(np.cov(a, b, bias=True)[0, 1] / b.var())
    assert cc_checker > 0.95 and 0.5 < covered.mean() < 1.0
    fit = first.compareMaps(second, operator=p["motion"])
    print("compareMaps: cc %.6f (checker %.6f), scale %.6f (checker %.6f), covered %.4f" % (fit["cc"], cc_checker, fit["scale"], scale_checker, fit["coveredFraction"]))
    assert fit["n"] == int(covered.sum()) and fit["coveredFraction"] == float(covered.mean()) and fit["rmsd"] is None
    assert fit["cc"] >= cc_checker - 1e-6 and abs(fit["scale"] - scale_checker) < 1e-6
    own = first.compareMaps(second)                      # the operator from the atoms: float32 coordinates move it by 1e-5 A
    assert own["rmsd"] < 1e-4 and abs(own["cc"] - fit["cc"]) < 1e-3


def test_isomorphous_difference_finds_the_planted_sites(pair):
    p, first, second = pair
    diff = first.isomorphousDifferenceObj(second, operator=p["motion"])
    grid = diff.density
    assert np.isfinite(grid).all() and list(diff.header.ncrs) == list(first.densityObj.header.ncrs)
    fit = first.compareMaps(second, operator=p["motion"])
    want, _ = chk.resample(p["second"][0], p["second"][1], p["first"][0], p["motion"], 1, fill=0.0, base=p["first"][1], alpha=-fit["scale"])
    assert_same_bits(grid, want, "the isomorphous difference map")
    green, red = diff.createFullBlobLists(0.5)            # a third of a planted site's height; the interpolation leaves less than 0.2
    assert len(green) == 0 and len(red) == len(p["planted"])
    for site in p["planted"]:
        assert min(float(np.linalg.norm(np.asarray(b.centroid) - site)) for b in red) < 0.25


def test_symmetry_expansion_restores_the_cell(gpu_ctx):
    """A P2-like cell: noise plus its own image under (x, y, z) -> (-x, -y, z) is symmetric to the bit.  A cut-out of a little more than
    half of it along c, expanded with the two operators at order 0, is the whole cell again."""
    from pdb_eda_amd import ccp4
    header, noise = rc.header_of("box"), rc.grid_of("box")
    full = noise + np.roll(noise[:, ::-1, ::-1], (1, 1), axis=(1, 2))
    nc = int(header.ncrs[0])
    cut = rc.window_header("box", (0, 0, 0), (nc // 2 + 2, header.ncrs[1], header.ncrs[2]))
    two_fold = np.hstack([np.diag([-1.0, -1.0, 1.0]), np.zeros((3, 1))])
    entry = _entry(gpu_ctx, "p2", cut, np.ascontiguousarray(full[:, :, :nc // 2 + 2]), np.zeros((3, 3)), rotation_mats=[ccp4.identityOperator(), two_fold])
    expanded = entry.densityObj.symmetryExpanded(entry.pdbObj.header.rotationMats, order=0)
    assert list(expanded.header.ncrs) == list(header.ncrs) and expanded.resampleCounters["uncovered"] == 0
    assert expanded.density.tobytes() == full.tobytes()
    assert entry.expandedDensityObj.density.tobytes() == full.tobytes()          # (order 1 on grid points: the same voxels)
    alone = entry.densityObj.resampled(ccp4.cellHeader(cut), order=0, fill=np.nan).density
    assert np.isnan(alone).mean() > 0.3                                            # the identity alone leaves the rest of the cell empty
