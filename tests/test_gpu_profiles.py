"""Radial density profiles on the MI355X path against tests/profiles_checker.py, the plain numpy restatement of the contract in
include/pdbeda.h (pdbeda_radial_profiles).  Shell membership is compared exactly (n, nSig, valid with np.array_equal; the
checker takes the voxel coordinates from the device's crs2xyz, which tests/test_gpu_voxel.py pins bit for bit); a shell's
density within 1e-9 * n[k] * max |rho|: the project's 1e-9 for fp64 sums, scaled by what the fixed-point quantum of the sums is
derived from (a voxel enters a sum rounded to a quantum of at most 2^-38 max |rho|, 4e-12)."""
import io
import json

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import profiles_cases
import profiles_checker

pytestmark = pytest.mark.gpu

SHAPES = [(1.0, 1), (2.0, 20), (3.5, 64)]          # (radius, nShells): one shell, the analysis default, the most shells


@pytest.fixture(scope="module", params=VOXEL_CASES)
def case(request, gpu_ctx):
    from pdb_eda_amd import ccp4
    z, header, grid = load_case(request.param)
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), request.param, ctx=gpu_ctx)
    return request.param, header, grid, dm, profiles_cases.case_atoms(request.param, header)


def assert_profiles_equal(got, want, grid, what):
    """got: DeviceMap.radial_profiles();  want: profiles_checker.radial_profiles()."""
    assert np.array_equal(got["n"], want["n"]), what
    assert np.array_equal(got["nSig"], want["n_sig"]), what
    assert np.array_equal(got["valid"], want["valid"]), what
    top = float(np.abs(grid).max())
    for mine, theirs, count in ((got["sum"], want["sum"], want["n"]), (got["sumSig"], want["sum_sig"], want["n_sig"])):
        err = np.abs(mine - theirs)
        bound = 1e-9 * count * top
        print("%s: max |sum - checker| = %.3g (bound at that shell %.3g), %d voxels in %d shells" %
              (what, float(err.max()), float(bound.reshape(-1)[int(err.argmax())]), int(count.sum()), count.size))
        assert np.all(err <= bound), what
        assert np.all(mine[count == 0] == 0.0), what          # an empty shell is exactly 0


@pytest.mark.parametrize("radius,n_shells", SHAPES)
def test_golden_maps_against_checker(case, radius, n_shells):
    name, header, grid, dm, xyz = case
    sigma = dm.meanDensity + 1.5 * dm.stdDensity
    for cut in (0.0, sigma, -sigma):
        got = dm._map.radial_profiles(xyz, radius, n_shells, cut)
        want = profiles_checker.radial_profiles(header, grid, xyz, radius, n_shells, cut, crs2xyz=dm._map.crs2xyz)
        assert got["n"].shape == (len(xyz), n_shells) and got["valid"].shape == (len(xyz),)
        assert_profiles_equal(got, want, grid, "%s r=%g shells=%d cut=%+.3g" % (name, radius, n_shells, cut))
        assert want["n"].sum() > 0
        if cut == 0.0:
            assert np.array_equal(got["nSig"], got["n"]) and np.array_equal(got["sumSig"].view(np.uint64), got["sum"].view(np.uint64))
        else:
            assert 0 < want["n_sig"].sum() < want["n"].sum()
        if name in ("orth_sub", "hex"):          # stored voxels missing from the cell: both answers occur, so `valid` is tested
            assert want["valid"].any() and not want["valid"].all()
    # the object model hands the same arrays on
    again = dm.radialProfiles([list(p) for p in xyz], radius, n_shells, -sigma)
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_voxels_exactly_on_shell_boundaries(gpu_ctx):
    """orth_rep has spacing 0.5: with radius 2.0 in 16 shells (w = 0.125 divides the spacing) dozens of the voxels around an
    atom on a voxel centre sit exactly on a shell boundary -- floor(d / w) decides, bit for bit."""
    from pdb_eda_amd import ccp4
    z, header, grid = load_case("orth_rep")
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), "orth_rep", ctx=gpu_ctx)
    xyz = profiles_cases.case_atoms("orth_rep", header, n_random=0, n_centres=8)
    sigma = dm.meanDensity + 1.5 * dm.stdDensity
    for cut in (0.0, sigma):
        want = profiles_checker.radial_profiles(header, grid, xyz, 2.0, 16, cut, crs2xyz=dm._map.crs2xyz)
        print("voxels exactly on a shell boundary, per atom: %s" % want["boundary_ties"].tolist())
        assert want["boundary_ties"].sum() >= 10 and np.all(want["boundary_ties"] >= 10)
        assert_profiles_equal(dm._map.radial_profiles(xyz, 2.0, 16, cut), want, grid, "orth_rep ties cut=%+.3g" % cut)


@pytest.mark.parametrize("name", ["orth", "tric"])
def test_consistent_with_region_sums(gpu_ctx, name):
    from pdb_eda_amd import ccp4
    z, header, grid = load_case(name)
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx)
    xyz = profiles_cases.case_atoms(name, header)
    sigma = dm.meanDensity + 1.5 * dm.stdDensity
    top = float(np.abs(grid).max())
    off = np.arange(len(xyz) + 1, dtype=np.int64)
    for radius, n_shells in SHAPES:
        rad = np.full(len(xyz), radius, dtype=np.float32)
        pos, neg, cnt, valid = dm._map.region_sums(xyz, rad, off, sigma)
        plus = dm._map.radial_profiles(xyz, radius, n_shells, sigma)
        minus = dm._map.radial_profiles(xyz, radius, n_shells, -sigma)
        assert np.array_equal(plus["n"].sum(1), cnt) and np.array_equal(minus["n"].sum(1), cnt)
        assert np.array_equal(plus["valid"], valid)
        print("%s r=%g: max |sum of shells - pos| = %.3g, - neg = %.3g" %
              (name, radius, float(np.abs(plus["sumSig"].sum(1) - pos).max()), float(np.abs(minus["sumSig"].sum(1) - neg).max())))
        assert np.all(np.abs(plus["sumSig"].sum(1) - pos) <= 1e-9 * plus["nSig"].sum(1) * top)
        assert np.all(np.abs(minus["sumSig"].sum(1) - neg) <= 1e-9 * minus["nSig"].sum(1) * top)
        if n_shells == 1:          # one shell IS the region: column for column
            assert np.array_equal(plus["n"][:, 0], cnt)
            assert np.all(np.abs(plus["sumSig"][:, 0] - pos) <= 1e-9 * plus["nSig"][:, 0] * top)
            assert np.all(np.abs(minus["sumSig"][:, 0] - neg) <= 1e-9 * minus["nSig"][:, 0] * top)


def test_bit_identical_from_run_to_run_and_across_batches(gpu_ctx):
    from pdb_eda_amd import ccp4
    z, header, grid = load_case("orth")
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), "orth", ctx=gpu_ctx)
    base = profiles_cases.case_atoms("orth", header, n_random=32, n_centres=8)
    xyz = np.tile(base, (8, 1))[:300]
    sigma = dm.meanDensity + 1.5 * dm.stdDensity
    first = dm._map.radial_profiles(xyz, 2.0, 20, sigma)
    second = dm._map.radial_profiles(xyz, 2.0, 20, sigma)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    a, b = dm._map.radial_profiles(xyz[:113], 2.0, 20, sigma), dm._map.radial_profiles(xyz[113:], 2.0, 20, sigma)
    for k in first:
        assert np.concatenate([a[k], b[k]]).tobytes() == first[k].tobytes(), k
    assert first["n"].sum() > 0 and np.array_equal(first["n"][:40], first["n"][40:80])


def test_arguments(gpu_ctx):
    from pdb_eda_amd import _native, ccp4
    z, header, grid = load_case("orth")
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), "orth", ctx=gpu_ctx)
    xyz = profiles_cases.case_atoms("orth", header)
    want = dm._map.radial_profiles(xyz, 2.0, 20, 0.0)
    bad_xyz = xyz.copy()
    bad_xyz[5, 1] = np.nan
    for args in ((xyz, 2.0, 0, 0.0), (xyz, 2.0, 65, 0.0), (xyz, 0.0, 20, 0.0), (xyz, np.inf, 20, 0.0), (bad_xyz, 2.0, 20, 0.0)):
        with pytest.raises(_native.PdbedaError):
            dm._map.radial_profiles(*args)
        again = dm._map.radial_profiles(xyz, 2.0, 20, 0.0)          # the context is not poisoned
        assert all(np.array_equal(again[k], want[k]) for k in want)
    empty = dm._map.radial_profiles(np.zeros((0, 3)), 2.0, 20, 0.0)
    assert empty["n"].shape == (0, 20) and empty["sum"].shape == (0, 20) and empty["nSig"].shape == (0, 20) and empty["sumSig"].shape == (0, 20)
    assert empty["valid"].shape == (0,)


# ---- the analysis surface ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analysis(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    return densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb), np.asarray(z["dens"], dtype=np.float32)


def test_analysis_tables(analysis):
    from pdb_eda_amd import densityAnalysis, singleStructure
    an, grid = analysis
    dm = an.densityObj
    header = an.atomRadialProfileHeader
    table = an.calculateAtomRadialProfiles(2.0, 20)
    atoms = list(an.biopdbObj.get_atoms())
    assert len(table) == len(atoms) and all(len(row) == len(header) for row in table)
    xyz = np.array([a.coord for a in atoms], dtype=np.float64)
    want = profiles_checker.radial_profiles(dm.header, grid, xyz, 2.0, 20, dm.meanDensity + 1.5 * dm.stdDensity, crs2xyz=dm._map.crs2xyz)
    col = {name: [row[k] for row in table] for k, name in enumerate(header)}
    got = {"n": np.array(col["shell_voxels"]), "sum": np.array(col["shell_density"]), "nSig": np.array(col["shell_significant_voxels"]),
           "sumSig": np.array(col["shell_significant_density"]), "valid": np.array(col["valid"])}
    assert_profiles_equal(got, want, grid, "analysis orth")
    types, electrons = densityAnalysis.fullAtomNameMapAtomTypeGlobal, densityAnalysis.fullAtomNameMapElectronsGlobal
    for row, atom in zip(table, atoms):
        r = dict(zip(header, row))
        full = densityAnalysis.residueAtomName(atom)
        assert r["atom_name"] == atom.name and r["bfactor"] == atom.get_bfactor() and r["occupancy"] == atom.get_occupancy()
        assert r["atom_type"] == types.get(full) and r["electrons"] == (electrons.get(full) if full in types else None)
    assert any(r is None for r in col["atom_type"]) or all(densityAnalysis.residueAtomName(a) in types for a in atoms)
    # per atom type: a numpy recomputation from the rows above
    ratio = an.densityElectronRatio
    assert ratio
    by_type = an.atomTypeRadialProfiles(2.0, 20)
    eligible = [i for i, a in enumerate(atoms) if a.parent.id[0] == ' ' and col["atom_type"][i] is not None and a.get_occupancy() != 0]
    assert [row[0] for row in by_type] == sorted({col["atom_type"][i] for i in eligible}) and len(by_type) >= 2
    width = float(np.float32(2.0)) / 20.0
    for row in by_type:
        r = dict(zip(an.atomTypeRadialProfileHeader, row))
        mine = [i for i in eligible if col["atom_type"][i] == r["atom_type"]]
        curves = np.array([np.cumsum(col["shell_significant_density"][i]) / col["electrons"][i] for i in mine])
        median = np.median(curves, axis=0)
        assert r["num_atoms"] == len(mine) and r["optimized_radius"] == densityAnalysis.radiiGlobal[r["atom_type"]]
        assert r["shell_outer_radius"] == [(k + 1) * width for k in range(20)]
        assert np.array_equal(np.array(r["median_cumulative_density_per_electron"]), median)
        reached = np.nonzero(median >= ratio)[0]
        assert r["profile_radius"] == ((int(reached[0]) + 1) * width if len(reached) else None)
    # `single` mode: both levels, through JSON and CSV
    for level, reference in (("atom", table), ("atom-type", by_type)):
        head, rows = singleStructure.rows(an, "profile", level, radius=2.0, shells=20)
        assert rows == reference
        assert json.loads(singleStructure.dumps(head, rows, "json")) == [dict(zip(head, row)) for row in rows]
        text = singleStructure.dumps(head, rows, "csv").splitlines()
        assert text[0] == ",".join(head) and text[1:] == [",".join(map(str, row)) for row in rows]
