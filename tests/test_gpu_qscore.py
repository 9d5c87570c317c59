"""Trilinear density and atom Q-scores on the MI355X path against tests/qscore_checker.py, the plain numpy restatement of the
contracts in include/pdbeda.h (pdbeda_interp_density, pdbeda_atom_qscores).  Every atom is compared.  shell_n, n_points and valid
are compared exactly (np.array_equal: the checker evaluates the sample points and the squared distances in the same unfused fp64);
shell_mean and the interpolated density within 1e-9 * max |rho| -- the project's bound for fp64 results --, q within 1e-9 absolute
(tests/test_qscore_host.py checks the conditioning of every seeded input used here)."""
import ctypes
import io
import json

import numpy as np
import pytest

from conftest import load_analysis_case, load_case
import qscore_cases
import qscore_checker

pytestmark = pytest.mark.gpu

QS_STAGE = qscore_cases.QS_STAGE
OUTPUTS = ("q", "nPoints", "shellN", "shellMean", "valid", "counters")
_maps, _wanted, _got = {}, {}, {}


def device_map(name, gpu_ctx):
    from pdb_eda_amd import ccp4
    if name not in _maps:
        z, header, grid = load_case(name)
        _maps[name] = (header, grid, ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx))
    return _maps[name]


def default_args(**kw):
    ref, unit, off = qscore_cases.tables(**kw)
    return (kw.get("step", qscore_cases.STEP), ref, unit, off, kw.get("points", qscore_cases.POINTS))


def wanted(key, header, grid, xyz, scored, args):
    """The checker's answer, computed once per input and shared (never modified)."""
    if key not in _wanted:
        _wanted[key] = qscore_checker.qscores(header, grid, xyz, scored, *args)
    return _wanted[key]


def golden(name, gpu_ctx):
    """(header, grid, map, atoms, the device's answer, the checker's) of a golden map with its seeded chain, every atom scored."""
    header, grid, dm = device_map(name, gpu_ctx)
    xyz = qscore_cases.chain(name, header)
    if name not in _got:
        _got[name] = dm._map.qscores(xyz, None, *default_args())
    return header, grid, dm, xyz, _got[name], wanted((name, "chain"), header, grid, xyz, None, default_args())


def assert_bits(a, b, what, keys=OUTPUTS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def assert_scores_equal(got, want, grid, what, counters=True):
    """got: DeviceMap.qscores();  want: qscore_checker.qscores()."""
    assert got["shellN"].dtype == np.int32 and got["nPoints"].dtype == np.int32 and got["q"].dtype == np.float64
    assert np.array_equal(got["shellN"], want["shell_n"]), what
    assert np.array_equal(got["nPoints"], want["n_points"]) and np.array_equal(got["nPoints"], got["shellN"].sum(axis=1)), what
    assert np.array_equal(got["valid"], want["valid"]), what
    top = float(np.abs(grid[np.isfinite(grid)]).max())
    err = np.abs(got["shellMean"] - want["shell_mean"])
    assert np.all(got["shellMean"][want["shell_n"] == 0] == 0.0), what          # an empty shell: exactly 0
    assert np.array_equal(np.isnan(got["q"]), np.isnan(want["q"])), what
    have = ~np.isnan(want["q"])
    dq = np.abs(got["q"][have] - want["q"][have])
    print("%s: %d atoms (%d with a score), max |shell_mean - checker| = %.3g (bound %.3g), max |q - checker| = %.3g, counters %s"
          % (what, len(want["q"]), int(have.sum()), float(err.max()), 1e-9 * top, float(dq.max()) if len(dq) else 0.0, got["counters"].tolist()))
    assert np.all(err <= 1e-9 * top), what
    assert np.all(dq <= 1e-9) and np.all(np.abs(got["q"][have]) <= 1.0), what
    if counters:
        assert got["counters"].tolist() == [int((want["neighbours"] > QS_STAGE).sum()), int(want["neighbours"].max())], what


# ---- the golden maps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qscore_cases.GOLDEN_MAPS)
def test_golden_maps_against_checker(gpu_ctx, name):
    header, grid, dm, xyz, got, want = golden(name, gpu_ctx)
    corners = qscore_cases.box_corners(header)
    frac = qscore_checker.frac(header, xyz)
    outside = int(np.any((frac < 0) | (frac > np.asarray(header.ncrs) - 1), axis=1).sum())
    escalated = int((want["shell_n"][:, 1:] > qscore_cases.POINTS).sum())
    print("%s: %d of %d atoms outside the stored box, %d shells went beyond level 0, %d empty shells, %d atoms not valid, most neighbours %d"
          % (name, outside, len(xyz), escalated, int((want["shell_n"] == 0).sum()), int((~want["valid"]).sum()), int(want["neighbours"].max())))
    assert len(xyz) == 300 and outside >= 10 and escalated >= 100 and (want["shell_n"] == 0).sum() >= 100          # (a vacuous comparison cannot pass)
    assert np.isfinite(want["q"]).sum() >= 200 and len(corners) == 8
    if name in ("orth_sub", "hex"):          # stored voxels missing from the cell: zeros and valid == 0, and both answers occur
        assert want["valid"].any() and not want["valid"].all()
    if not header.orthogonal:
        assert want["near_integer"] > 1e-9
    assert_scores_equal(got, want, grid, name)
    again = dm.qScores([list(p) for p in xyz])          # the object model makes the same tables and hands the same arrays on
    assert_bits(again, got, name)


@pytest.mark.parametrize("name", qscore_cases.GOLDEN_MAPS)
def test_interpolated_density_against_checker(gpu_ctx, name):
    header, grid, dm = device_map(name, gpu_ctx)
    rng = np.random.default_rng(len(name) + 17)
    ncrs = np.asarray(header.ncrs, dtype=np.float64)
    xyz = np.concatenate([qscore_cases.chain(name, header), header.crs2xyz_array(rng.uniform(-1.5 * ncrs, 2.5 * ncrs, size=(400, 3)))])
    values, valid, f = qscore_checker.interp(header, grid, xyz)
    if not header.orthogonal:
        assert np.abs(f - np.rint(f)).min() > 1e-9
    got, got_valid = dm._map.interp_density(xyz)
    top = float(np.abs(grid).max())
    print("%s: %d points, %d valid, max |interpolated - checker| = %.3g (bound %.3g)" % (name, len(xyz), int(valid.sum()), float(np.abs(got - values).max()), 1e-9 * top))
    assert got.dtype == np.float64 and got_valid.dtype == bool and 0 < valid.sum()
    assert np.array_equal(got_valid, valid) and np.all(np.abs(got - values) <= 1e-9 * top)
    if name in ("orth_sub", "hex"):
        assert not valid.all() and np.any(got[~valid] == 0.0)
    many = dm.getInterpolatedDensityFromXyz([list(p) for p in xyz[:5]])
    assert many.tobytes() == got[:5].tobytes() and dm.getInterpolatedDensityFromXyz(list(xyz[3])) == got[3] and isinstance(dm.getInterpolatedDensityFromXyz(xyz[3]), float)


def test_interpolated_density_on_both_sides_of_a_block(gpu_ctx):
    """One thread per point in blocks of 256, no cap on the grid: 1, 255, 256, 257 and 513 points."""
    header, grid, dm = device_map("tric", gpu_ctx)
    rng = np.random.default_rng(3)
    xyz = header.crs2xyz_array(rng.uniform(-2.0, np.asarray(header.ncrs, dtype=np.float64) + 2.0, size=(513, 3)))
    values, valid, _ = qscore_checker.interp(header, grid, xyz)
    for n in (1, 255, 256, 257, 513):
        got, got_valid = dm._map.interp_density(xyz[:n])
        assert len(got) == n and np.array_equal(got_valid, valid[:n]) and np.all(np.abs(got - values[:n]) <= 1e-9 * float(np.abs(grid).max())), n
    empty, empty_valid = dm._map.interp_density(np.zeros((0, 3)))
    assert empty.shape == (0,) and empty_valid.shape == (0,)


def test_voxel_centres_faces_and_exact_ties(gpu_ctx):
    """orth_rep has spacing 0.5 (exact in binary).  On voxel centres -- inside the stored box, on its faces and beyond them, where the
    map wraps -- the interpolant IS point_density, to the bit (the positions are checked to come out as integers: the origin's x is an ulp
    off 1.0, and column 1 alone does not).  With axis directions and a step of 0.5 every sample point is a voxel
    centre too, and a competitor at 2 R along an axis is exactly as far from the sample point as the atom: it rejects nothing."""
    header, grid, dm = device_map("orth_rep", gpu_ctx)
    nc, nr, ns = (int(v) for v in header.ncrs)
    crs = np.array([[c, r, s] for c in (-3, 0, 2, nc - 1, nc, nc + 2) for r in (-1, 0, 7, nr - 1, nr + 1) for s in (-2, 0, 5, ns - 1, ns)], dtype=np.int32)
    xyz = np.array([header.crs2xyzCoord([int(v) for v in c]) for c in crs], dtype=np.float64)
    got, valid = dm._map.interp_density(xyz)
    assert np.array_equal(got, dm._map.point_density(crs)) and np.any(got != 0.0)
    want_values, want_valid, f = qscore_checker.interp(header, grid, xyz)
    assert np.array_equal(f, crs.astype(np.float64)) and np.array_equal(valid, want_valid) and np.array_equal(got, want_values)
    axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    ref = np.array([1.0, 0.7, 0.4, 0.2])
    atom = np.array(header.crs2xyzCoord([12, 11, 10]), dtype=np.float64)
    atoms = np.array([atom, atom + [1.0, 0, 0], atom + [0, -2.0, 0], atom + [0, 0, 3.0], atom + [0.25, 0.25, 5.0]])
    args = (0.5, ref, axes, np.array([0, 6], dtype=np.int32), 1)
    want = qscore_checker.qscores(header, grid, atoms, [0], *args)
    # shell 1 (R 0.5) ties with the atom at +1.0 x and keeps all six points; on shell 2 (R 1.0) that atom sits ON the +x point and takes it,
    # the atom at -2.0 y ties; on shell 3 (R 1.5) the +x and -y points are lost, the atom at +3.0 z ties
    assert want["shell_n"].tolist() == [[1, 6, 5, 4]]
    got = dm._map.qscores(atoms, [0], *args)
    assert_scores_equal(got, want, grid, "orth_rep ties")
    centre = float(dm._map.point_density(np.array([[12, 11, 10]], dtype=np.int32))[0])
    ring = dm._map.point_density(np.array([[13, 11, 10], [11, 11, 10], [12, 12, 10], [12, 10, 10], [12, 11, 11], [12, 11, 9]], dtype=np.int32))
    assert got["shellMean"][0, 0] == centre and abs(got["shellMean"][0, 1] - ring.mean()) <= 1e-13 * np.abs(ring).max()


# ---- crafted neighbourhoods ------------------------------------------------------------------------------------------------------
def test_crafted_neighbourhoods(gpu_ctx):
    """The smallest inputs that reach each branch of the shell rule, far enough apart (12 A) not to see each other; orth stores its
    whole cell, so every point is valid wherever the atoms sit."""
    header, grid, dm = device_map("orth", gpu_ctx)
    at = qscore_cases.middle(header) + np.array([0.07, 0.02, -0.04])
    far = lambda k: at + np.array([12.0 * k, 0.0, 0.0])
    six = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    groups = [("isolated", far(0)[None, :]),
              ("pair", np.array([far(1), far(1) + [1.5, 0, 0]])),
              ("coincident", np.array([far(2), far(2), far(2)])),
              ("boxed", np.concatenate([far(3)[None, :], far(3) + 1.2 * six, far(3) + 1.2 * np.array([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, 1, 1], [-1, 1, -1], [-1, -1, 1], [-1, -1, -1]]) / np.sqrt(3.0)])),
              ("smothered", np.concatenate([far(4)[None, :], far(4) + 0.05 * six]))]
    xyz = np.concatenate([g for _, g in groups])
    first = dict(zip([n for n, _ in groups], np.cumsum([0] + [len(g) for _, g in groups])[:-1].tolist()))
    args = default_args()
    want = wanted(("orth", "crafted"), header, grid, xyz, None, args)
    full = [1] + [qscore_cases.POINTS] * 20
    assert want["shell_n"][first["isolated"]].tolist() == full
    pair = want["shell_n"][first["pair"]]
    assert pair[:7].tolist() == full[:7] and pair.max() > qscore_cases.POINTS and want["shell_n"][first["pair"] + 1].max() > qscore_cases.POINTS          # the levels escalate
    for k in range(3):          # ties keep the points
        assert want["shell_n"][first["coincident"] + k].tolist() == full
    boxed = want["shell_n"][first["boxed"]]
    assert boxed[-1] == 0 and boxed[1] == qscore_cases.POINTS and want["n_points"][first["boxed"]] > 1 and np.isfinite(want["q"][first["boxed"]])          # nothing at the last level
    assert want["shell_n"][first["smothered"]].tolist() == [1] + [0] * 20 and want["n_points"][first["smothered"]] == 1 and np.isnan(want["q"][first["smothered"]])
    got = dm._map.qscores(xyz, None, *args)
    assert_scores_equal(got, want, grid, "orth crafted")
    assert got["valid"].all()
    for k in (1, 2):          # coincident atoms: the same numbers, to the bit
        for name in ("q", "shellMean", "shellN", "nPoints"):
            assert got[name][first["coincident"] + k].tobytes() == got[name][first["coincident"]].tobytes()


@pytest.mark.parametrize("extra,overflowed", [(QS_STAGE - 4, 0), (QS_STAGE - 3, 1), (3 * QS_STAGE - 4, 1)])
def test_staging_buffer_edges(gpu_ctx, extra, overflowed):
    """Atom 0 has exactly QS_STAGE, QS_STAGE + 1 and 3 * QS_STAGE neighbours: four bonded atoms and ``extra`` atoms just inside the reach
    that are too far to win any of its points.  The staged path and the cell walk must both equal the checker, say which of them ran,
    and give atom 0 the bits it gets when the extra atoms sit just outside the reach (where nothing stages or walks them)."""
    header, grid, dm = device_map("orth", gpu_ctx)
    near, far = qscore_cases.crowded(header, extra), qscore_cases.crowded(header, extra, far=True)
    args = default_args()
    scored = np.arange(5, dtype=np.int32)
    want = wanted(("orth", "crowded", extra), header, grid, near, scored, args)
    assert want["neighbours"][0] == 4 + extra and want["neighbours"][0] == want["neighbours"].max() and want["shell_n"][0].max() > qscore_cases.POINTS
    got = dm._map.qscores(near, scored, *args)
    assert_scores_equal(got, want, grid, "orth crowded %d" % extra)
    alone = dm._map.qscores(near, [0], *args)
    assert alone["counters"].tolist() == [overflowed, 4 + extra]
    apart = dm._map.qscores(far, [0], *args)
    assert apart["counters"].tolist() == [0, 4]
    assert_bits(alone, apart, "crowded %d against the same atoms outside the reach" % extra, keys=("q", "nPoints", "shellN", "shellMean", "valid"))
    assert_bits({k: v[:1] for k, v in got.items()}, alone, "crowded %d" % extra, keys=("q", "nPoints", "shellN", "shellMean", "valid"))


# ---- launch shapes and parameters ------------------------------------------------------------------------------------------------
def test_scored_subsets_orders_and_repeats(gpu_ctx):
    """Four atoms a workgroup: 1, 3, 4 and 5 scored atoms, any order, repeats -- each row is the row of the atom when all are scored."""
    header, grid, dm, xyz, base, want = golden("orth", gpu_ctx)
    args = default_args()
    for scored in ([0], [5, 6, 7], [0, 1, 2, 3], [296, 297, 298, 299, 0], [7, 3, 3, 299, 0, 7, 150, 3, 42]):
        got = dm._map.qscores(xyz, scored, *args)
        for mine in ("q", "nPoints", "shellN", "shellMean", "valid"):
            assert got[mine].tobytes() == base[mine][scored].tobytes(), (scored, mine)
        assert got["counters"].tolist() == [int((want["neighbours"][scored] > QS_STAGE).sum()), int(want["neighbours"][scored].max())]
    sub = dm.qScores(xyz, scored=[4, 2])
    assert sub["q"].tobytes() == base["q"][[4, 2]].tobytes()


@pytest.mark.parametrize("tag,kw,n_atoms", [("one atom", {}, 1), ("two shells", {"shells": 2}, 60), ("one level of 64", {"points": 64, "levels": 1}, 60),
                                            ("two levels, a step of 0.17", {"points": 5, "levels": 2, "step": 0.17, "shells": 9}, 60)])
def test_parameter_edges(gpu_ctx, tag, kw, n_atoms):
    header, grid, dm = device_map("hex", gpu_ctx)
    xyz = qscore_cases.chain("hex", header)[:n_atoms]
    args = default_args(**kw)
    want = wanted(("hex", tag), header, grid, xyz, None, args)
    if n_atoms == 1:
        assert want["shell_n"].tolist() == [[1] + [qscore_cases.POINTS] * 20] and want["neighbours"].tolist() == [0]
    assert want["near_integer"] > 1e-9
    assert_scores_equal(dm._map.qscores(xyz, None, *args), want, grid, "hex " + tag)


def test_min_points_of_one(gpu_ctx):
    header, grid, dm = device_map("orth_perm", gpu_ctx)
    xyz = qscore_cases.chain("orth_perm", header)[:80]
    step, ref, unit, off, _ = default_args()
    want = wanted(("orth_perm", "min 1"), header, grid, xyz, None, (step, ref, unit, off, 1))
    eight = wanted(("orth_perm", "min 8"), header, grid, xyz, None, (step, ref, unit, off, 8))
    assert (want["shell_n"] != eight["shell_n"]).sum() >= 50          # (a shell with one survivor at level 0 stops there)
    assert_scores_equal(dm._map.qscores(xyz, None, step, ref, unit, off, 1), want, grid, "orth_perm min_points 1")


def test_bit_identical_from_run_to_run_and_under_permutation(gpu_ctx):
    header, grid, dm, xyz, base, want = golden("wide", gpu_ctx)
    args = default_args()
    assert_bits(dm._map.qscores(xyz, None, *args), base, "wide, the same call again")
    perm = np.random.default_rng(11).permutation(len(xyz))
    place = np.argsort(perm)          # atom i of xyz is atom place[i] of xyz[perm]
    moved = dm._map.qscores(xyz[perm], place.astype(np.int32), *args)
    assert_bits(moved, base, "wide, competitors permuted and scored re-mapped")


# ---- refusals and empty inputs ---------------------------------------------------------------------------------------------------
def _raw_qscores(dm, xyz, n_all, scored, n_scored, step, n_shells, ref, unit, off, n_levels, min_points, outputs=None):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    out = outputs or [None] * 6
    return dm._map._ctx._lib.pdbeda_atom_qscores(dm._map._h, p(xyz), n_all, p(scored), n_scored, ctypes.c_float(step), n_shells, p(ref), p(unit), p(off), n_levels, min_points,
                                                 *[p(o) for o in out])


def test_arguments(gpu_ctx):
    from pdb_eda_amd import _native
    header, grid, dm, xyz, base, want = golden("orth", gpu_ctx)
    xyz = xyz[:40]
    step, ref, unit, off, points = default_args()
    good = dm._map.qscores(xyz, None, step, ref, unit, off, points)
    good_values, good_valid = dm._map.interp_density(xyz)

    def still_fine():          # the context is not poisoned
        assert_bits(dm._map.qscores(xyz, None, step, ref, unit, off, points), good, "a good call after a refusal")
        again, again_valid = dm._map.interp_density(xyz)
        assert again.tobytes() == good_values.tobytes() and np.array_equal(again_valid, good_valid)

    def with_value(array, index, value):
        changed = np.array(array, dtype=np.float64, copy=True)
        changed[index] = value
        return changed

    beyond = np.array(header.crs2xyzCoord([2 ** 29 + 10, 0, 0]), dtype=np.float64)
    bad_calls = [("step 0", (xyz, None, 0.0, ref, unit, off, points)), ("step < 0", (xyz, None, -0.1, ref, unit, off, points)),
                 ("step nan", (xyz, None, np.nan, ref, unit, off, points)), ("step inf", (xyz, None, np.inf, ref, unit, off, points)),
                 ("one shell", (xyz, None, step, ref[:1], unit, off, points)), ("65 shells", (xyz, None, step, np.linspace(1.0, 0.0, 65), unit, off, points)),
                 ("nine levels", (xyz, None, step, ref, unit, np.arange(10, dtype=np.int32), 1)),
                 ("an empty level", (xyz, None, step, ref, unit, np.array([0, 8, 8, 24], dtype=np.int32), points)),
                 ("a level of 65", (xyz, None, step, ref, unit, np.array([0, 8, 73], dtype=np.int32), points)),
                 ("offsets from 1", (xyz, None, step, ref, unit, np.array([1, 9], dtype=np.int32), points)),
                 ("min_points 0", (xyz, None, step, ref, unit, off, 0)), ("min_points above level 0", (xyz, None, step, ref, unit, off, points + 1)),
                 ("ref nan", (xyz, None, step, with_value(ref, 3, np.nan), unit, off, points)), ("unit inf", (xyz, None, step, ref, with_value(unit, (100, 1), np.inf), off, points)),
                 ("coordinate nan", (with_value(xyz, (7, 2), np.nan), None, step, ref, unit, off, points)),
                 ("competitor inf", (with_value(xyz, (39, 0), -np.inf), [0, 1], step, ref, unit, off, points)),
                 ("scored -1", (xyz, [0, -1], step, ref, unit, off, points)), ("scored n_all", (xyz, [3, len(xyz)], step, ref, unit, off, points)),
                 ("a scored atom 2^29 steps away", (np.concatenate([xyz, beyond[None, :]]), [len(xyz)], step, ref, unit, off, points)),
                 ("a step of 1e9", (xyz, None, 1e9, ref, unit, off, points))]
    for what, args in bad_calls:
        with pytest.raises(_native.PdbedaError) as info:
            dm._map.qscores(*args)
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT, what
        still_fine()
    far_competitor = dm._map.qscores(np.concatenate([xyz, beyond[None, :]]), np.arange(len(xyz), dtype=np.int32), step, ref, unit, off, points)          # only SCORED atoms are sampled
    assert_bits(far_competitor, good, "a competitor 2^29 steps away", keys=("q", "nPoints", "shellN", "shellMean", "valid"))
    # raw calls: no level at all, 2^31 atoms (refused before the coordinates are read: no array of that length exists)
    for what, rc in (("no level", _raw_qscores(dm, xyz, len(xyz), None, 0, step, len(ref), ref, unit, off, 0, 1)),
                     ("2^31 atoms", _raw_qscores(dm, xyz, 2 ** 31, None, 0, step, len(ref), ref, unit, off, len(off) - 1, points)),
                     ("2^31 scored", _raw_qscores(dm, xyz, len(xyz), np.zeros(4, dtype=np.int32), 2 ** 31, step, len(ref), ref, unit, off, len(off) - 1, points))):
        with pytest.raises(_native.PdbedaError) as info:
            dm._map._ctx.check(rc, "pdbeda_atom_qscores")
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT, what
        still_fine()
    # the interpolated density: a non-finite coordinate and one 2^29 steps away, named by its index
    for what, points_in, index in (("nan", with_value(xyz, (11, 1), np.nan), 11), ("inf", with_value(xyz, (0, 0), np.inf), 0), ("2^29 steps", np.concatenate([xyz, beyond[None, :]]), len(xyz))):
        with pytest.raises(_native.PdbedaError) as info:
            dm._map.interp_density(points_in)
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT and ("point %d " % index) in str(info.value), what
        still_fine()
    inside = np.array(header.crs2xyzCoord([2 ** 29 - 10, 0, 0]), dtype=np.float64)          # just below the limit: wrapped like any other point
    value, valid = dm._map.interp_density(inside[None, :])
    assert valid[0] and abs(value[0] - qscore_checker.interp(header, grid, inside[None, :])[0][0]) <= 1e-9 * float(np.abs(grid).max())


def test_empty_inputs_touch_nothing(gpu_ctx):
    header, grid, dm, xyz, base, want = golden("orth", gpu_ctx)
    step, ref, unit, off, points = default_args()
    canary = [np.full(2, 7.5), np.full(2, 7, np.int32), np.full((2, 21), 7, np.int32), np.full((2, 21), 7.5), np.full(2, 7, np.uint8), np.full(2, 7, np.int64)]
    for what, rc in (("no scored atom", _raw_qscores(dm, xyz, len(xyz), np.zeros(1, dtype=np.int32), 0, step, len(ref), ref, unit, off, len(off) - 1, points, canary)),
                     ("no atom at all", _raw_qscores(dm, None, 0, None, 0, step, len(ref), ref, unit, off, len(off) - 1, points, canary))):
        assert rc == 0, what
        assert all(np.all(c == c.dtype.type(7.5 if c.dtype == np.float64 else 7)) for c in canary), what
    out = dm._map.qscores(xyz, np.zeros(0, dtype=np.int32), step, ref, unit, off, points)
    assert out["q"].shape == (0,) and out["shellN"].shape == (0, 21)
    only_q = [np.zeros(3), None, None, None, None, None]          # any output may be NULL
    assert _raw_qscores(dm, xyz, len(xyz), np.array([2, 0, 1], dtype=np.int32), 3, step, len(ref), ref, unit, off, len(off) - 1, points, only_q) == 0
    assert only_q[0].tobytes() == base["q"][[2, 0, 1]].tobytes()
    lib, h = dm._map._ctx._lib, dm._map._h
    pts = np.ascontiguousarray(xyz[:9])
    values, flags = np.zeros(9), np.zeros(9, dtype=np.uint8)
    assert lib.pdbeda_interp_density(h, pts.ctypes.data_as(ctypes.c_void_p), 9, values.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert lib.pdbeda_interp_density(h, pts.ctypes.data_as(ctypes.c_void_p), 9, None, flags.ctypes.data_as(ctypes.c_void_p)) == 0
    both, both_flags = dm._map.interp_density(pts)
    assert values.tobytes() == both.tobytes() and np.array_equal(flags.astype(bool), both_flags)
    assert lib.pdbeda_interp_density(h, None, 0, None, None) == 0


# ---- the analysis surface --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["orth", "hex", "alias"])
def test_analysis_tables(gpu_ctx, name):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis, singleStructure
    z, spec, st, pdb, params = load_analysis_case(name)
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), name, ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), name, ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    an = densityAnalysis.DensityAnalysis(name, dens, diff, st, pdb)
    grid = np.asarray(z["dens"], dtype=np.float32).reshape(dens.header.ncrs[2], dens.header.ncrs[1], dens.header.ncrs[0])
    sym = an.symmetryAtoms
    coords = np.asarray(an.symmetryAtomCoords, dtype=np.float64)
    own = np.nonzero(sym._ident)[0]
    want = qscore_checker.qscores(dens.header, grid, coords, own, *default_args())
    if not dens.header.orthogonal:
        assert want["near_integer"] > 1e-9
    if name == "alias":          # atoms that share a coordinate tie everywhere and take nothing from each other
        twins = [k for k, j in enumerate(own) if (np.abs(coords - coords[j]).sum(axis=1) == 0).sum() > 1]
        assert len(twins) >= 2 and all(want["n_points"][k] > 1 for k in twins)
    atoms = list(an.biopdbObj.get_atoms())
    row_of = {int(sym._idx[j]): k for k, j in enumerate(own)}          # structure atom -> its row of the checker's answer
    header = an.atomQScoreHeader
    table = an.calculateAtomQScores()
    assert len(table) == len(atoms) and all(len(row) == len(header) for row in table) and len(row_of) > 0.5 * len(atoms)
    assert [row[:6] for row in table] == [row[:6] for row in an.calculateAtomRegionDensity(1.0)]
    worst, scores = 0.0, {}
    for k, row in enumerate(table):
        r = dict(zip(header, row))
        j = row_of.get(k)
        assert r["bfactor"] == atoms[k].get_bfactor()
        if j is None:
            assert r["q_score"] is None and r["n_points"] == 0 and r["valid"] is False
            continue
        assert r["n_points"] == int(want["n_points"][j]) and r["valid"] == bool(want["valid"][j])
        if np.isnan(want["q"][j]):
            assert r["q_score"] is None
        else:
            worst = max(worst, abs(r["q_score"] - want["q"][j]))
            scores[k] = r["q_score"]
    print("%s: %d of %d atoms have a score, max |q - checker| = %.3g, mean Q %.4f, counters %s" % (name, len(scores), len(atoms), worst, float(np.mean(list(scores.values()))), an._qScores[3].tolist()))
    assert worst <= 1e-9 and len(scores) > 0.5 * len(atoms)
    assert an._qScores[3].tolist() == [int((want["neighbours"] > QS_STAGE).sum()), int(want["neighbours"].max())]
    typed = an.calculateAtomQScores(type="CA")
    assert typed == [row for row in table if row[4] == "CA"] and len(typed) > 0
    # residues: mean and minimum over their atoms that have a score
    by_residue = an.calculateResidueQScores()
    residues = list(an.biopdbObj.get_residues())
    assert len(by_residue) == len(residues) and [row[:5] for row in by_residue] == [row[:5] for row in an.calculateResidueRegionDiscrepancies(1.0)]
    at = 0
    for row, residue in zip(by_residue, residues):
        mine = [scores[k] for k in range(at, at + len(residue)) if k in scores]
        at += len(residue)
        assert row[7] == len(mine)
        if mine:
            assert abs(row[5] - np.mean(mine)) <= 1e-12 and row[6] == min(mine)
        else:
            assert row[5] is None and row[6] is None
    assert at == len(atoms)
    # the summary: classes of atoms by name and residue kind
    summary = an.qScoreSummary()
    classes = {"all": [], "backbone": [], "side_chain": [], "water": []}
    for k, atom in enumerate(atoms):
        if k not in scores:
            continue
        residue = atom.parent
        classes["all"].append(scores[k])
        if residue.id[0] == " ":
            classes["backbone" if atom.name in ("N", "CA", "C", "O") else "side_chain"].append(scores[k])
        if residue.resname in ("HOH", "WAT", "DOD"):
            classes["water"].append(scores[k])
    assert len(classes["backbone"]) > 0 and len(classes["side_chain"]) > 0
    for cls, mine in classes.items():
        assert summary[cls + "_num_atoms"] == len(mine)
        if mine:
            assert abs(summary[cls + "_mean_q_score"] - np.mean(mine)) <= 1e-12 and abs(summary[cls + "_median_q_score"] - np.median(mine)) <= 1e-12
        else:
            assert summary[cls + "_mean_q_score"] is None and summary[cls + "_median_q_score"] is None
    # `single` mode: the three levels, through JSON and CSV
    for level, reference in (("atom", table), ("residue", by_residue), ("summary", None)):
        head, rows = singleStructure.rows(an, "qscore", level)
        if reference is not None:
            assert rows == reference
        else:
            assert len(rows) == 1 and dict(zip(head, rows[0])) == summary
        assert len(rows) > 0 and all(len(row) == len(head) for row in rows)
        assert json.loads(singleStructure.dumps(head, rows, "json")) == [dict(zip(head, row)) for row in rows]
        text = singleStructure.dumps(head, rows, "csv").splitlines()
        assert text[0] == ",".join(head) and text[1:] == [",".join(map(str, row)) for row in rows]
    with pytest.raises(ValueError):
        singleStructure.rows(an, "qscore", "domain")
