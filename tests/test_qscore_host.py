"""The Q-score and trilinear contracts without a GPU: facts about the numpy checker (tests/qscore_checker.py, the yardstick of
tests/test_gpu_qscore.py) and the host-made tables, the new names of the C-ABI in the header, the built library and the ctypes stub,
the new mode -- and, once for every seeded input the GPU tests compare, the conditioning of the correlations they compare."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_case
import qscore_cases
import qscore_checker


def _synthetic(ncrs, spacing, grid_of):
    from pdb_eda_amd import ccp4, synthetic
    header = ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(synthetic.MapSpec(ncrs=ncrs, spacing=spacing)))
    c, r, s = np.meshgrid(np.arange(ncrs[0]), np.arange(ncrs[1]), np.arange(ncrs[2]), indexing="ij")
    grid = np.ascontiguousarray(np.transpose(grid_of(c, r, s), (2, 1, 0)).astype(np.float32))          # [s][r][c]
    return header, grid


@pytest.mark.parametrize("n", [1, 2, 8, 16, 32, 64, 100])
def test_sphere_lattice(n):
    from pdb_eda_amd import ccp4
    u = ccp4.sphereLattice(n)
    assert u.shape == (n, 3) and u.dtype == np.float64
    assert np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 1e-15 and abs(u[:, 2].mean()) <= 1e-15
    assert len(np.unique(u.round(12), axis=0)) == n


def test_tables():
    from pdb_eda_amd import ccp4
    ref, unit, off = ccp4.qScoreTables()
    step32 = float(np.float32(0.1))
    assert off.tolist() == [0, 8, 24, 56, 120] and off.dtype == np.int32 and unit.shape == (120, 3) and len(ref) == 21
    assert ref[0] == 1.0 and np.array_equal(ref, np.exp(-0.5 * (np.arange(21) * step32 / 0.6) ** 2)) and np.all(np.diff(ref) < 0)
    assert np.array_equal(unit[24:56], ccp4.sphereLattice(32))
    ref, unit, off = ccp4.qScoreTables(0.5, 0.2, 6, 3, 2)
    assert off.tolist() == [0, 3, 9] and len(ref) == 6 and ref[1] == np.exp(-0.5 * (float(np.float32(0.2)) / 0.5) ** 2)


def test_interpolant_reproduces_a_linear_map_and_the_voxels():
    header, grid = _synthetic((12, 10, 9), 0.5, lambda c, r, s: 0.25 * c - 0.5 * r + 0.125 * s + 1.0)
    rng = np.random.default_rng(5)
    pos = rng.uniform([0, 0, 0], [11, 9, 8], size=(500, 3))                     # inside the stored box: no wrap across the ramp's jump
    xyz = header.crs2xyz_array(pos)
    values, valid, f = qscore_checker.interp(header, grid, xyz)
    want = 0.25 * pos[:, 0] - 0.5 * pos[:, 1] + 0.125 * pos[:, 2] + 1.0
    span = float(grid.max() - grid.min())
    print("linear map: max |interpolant - plane| = %.3g of a range of %.3g" % (float(np.abs(values - want).max()), span))
    assert valid.all() and np.abs(f - pos).max() <= 1e-12 and np.abs(values - want).max() <= 1e-12 * span
    # at integer positions the interpolant IS the voxel (spacing 0.5: crs2xyz and back are exact)
    crs = np.stack([rng.integers(0, 12, 200), rng.integers(0, 10, 200), rng.integers(0, 9, 200)], axis=1)
    values, valid, f = qscore_checker.interp(header, grid, np.array([header.crs2xyzCoord([int(v) for v in c]) for c in crs]))
    assert np.array_equal(f, crs.astype(np.float64)) and valid.all()
    assert np.array_equal(values, grid[crs[:, 2], crs[:, 1], crs[:, 0]].astype(np.float64))


def test_wrap_and_unstored_corners():
    """orth_sub stores a part of its cell: a point beside the stored box reads zeros and is not valid; orth_rep stores more than a
    cell: a point outside the stored box reads its periodic image."""
    z, header, grid = load_case("orth_sub")
    edge = np.array(header.crs2xyzCoord([int(header.ncrs[0]) - 1, 5, 5]), dtype=np.float64)
    step = np.array(header.crs2xyzCoord([int(header.ncrs[0]), 5, 5]), dtype=np.float64) - edge
    values, valid, _ = qscore_checker.interp(header, grid, np.array([edge + 0.25 * step, edge + 0.5 * step, edge + 1.5 * step]))
    last, tiny = float(grid[5, 5, -1]), 1e-12 * float(np.abs(grid).max())          # (spacing 0.4 is not exact in binary: the positions are voxels to a few ulps)
    assert valid.tolist() == [False, False, False] and abs(values[0] - 0.75 * last) <= tiny and abs(values[1] - 0.5 * last) <= tiny and values[2] == 0.0
    z, header, grid = load_case("orth_rep")
    inside = np.array(header.crs2xyzCoord([3, 4, 5]), dtype=np.float64) + 0.1
    shift = np.array(header.crs2xyzCoord([3 - int(header.crsInterval[0]), 4, 5]), dtype=np.float64) - np.array(header.crs2xyzCoord([3, 4, 5]), dtype=np.float64)
    values, valid, _ = qscore_checker.interp(header, grid, np.array([inside, inside + shift]))
    assert valid.all() and abs(values[0] - values[1]) <= 1e-12 * float(np.abs(grid).max())


def _one_atom(grid_of, spacing=0.25, ncrs=(40, 40, 40)):
    header, grid = _synthetic(ncrs, spacing, grid_of)
    ref, unit, off = qscore_cases.tables()
    atom = np.array([header.crs2xyzCoord([20, 20, 20])], dtype=np.float64) + [[0.03, -0.05, 0.07]]
    return header, grid, atom, (qscore_cases.STEP, ref, unit, off, qscore_cases.POINTS)


def test_q_is_invariant_under_scale_and_offset_and_flips_with_the_sign():
    z, header, grid = load_case("orth")
    xyz = qscore_cases.chain("orth", header)[:40]
    ref, unit, off = qscore_cases.tables()
    args = (qscore_cases.STEP, ref, unit, off, qscore_cases.POINTS)
    base = qscore_checker.qscores(header, grid.astype(np.float64), xyz, None, *args)
    moved = qscore_checker.qscores(header, 3.5 * grid.astype(np.float64) + 0.75, xyz, None, *args)
    flipped = qscore_checker.qscores(header, -2.0 * grid.astype(np.float64) + 0.1, xyz, None, *args)
    assert np.isfinite(base["q"]).all() and np.array_equal(base["shell_n"], moved["shell_n"]) and np.array_equal(base["shell_n"], flipped["shell_n"])
    print("alpha rho + beta: max |dq| = %.3g; sign flip: max |q + q'| = %.3g" % (float(np.abs(base["q"] - moved["q"]).max()), float(np.abs(base["q"] + flipped["q"]).max())))
    assert np.abs(base["q"] - moved["q"]).max() <= 1e-12 and np.abs(base["q"] + flipped["q"]).max() <= 1e-12 and np.abs(base["q"]).max() > 0.1


def test_a_constant_map_has_no_score():
    header, grid, atom, args = _one_atom(lambda c, r, s: 0.0 * c + 0.375)
    got = qscore_checker.qscores(header, grid, atom, None, *args)
    assert np.isnan(got["q"][0]) and got["n_points"][0] == 1 + 20 * 8 and np.all(got["shell_mean"][0] == 0.375)


def test_an_isolated_atom_on_its_own_gaussian_scores_high():
    """The map IS exp(-r^2 / (2 0.6^2)) around the atom, sampled at 0.25 A: the trilinear error is at most h^2 / 8 |f''| (about 2 % of
    the peak) and smooth, so the correlation loses less than 1e-3."""
    centre = np.array([20.12, 19.8, 20.28])          # (in voxels; the atom is put there below)
    header, grid = _synthetic((40, 40, 40), 0.25, lambda c, r, s: np.exp(-(0.25 ** 2) * ((c - centre[0]) ** 2 + (r - centre[1]) ** 2 + (s - centre[2]) ** 2) / (2 * 0.6 ** 2)))
    atom = header.crs2xyz_array(centre[None, :])
    ref, unit, off = qscore_cases.tables()
    got = qscore_checker.qscores(header, grid, atom, None, qscore_cases.STEP, ref, unit, off, qscore_cases.POINTS)
    print("isolated atom on its own Gaussian at 0.25 A: Q = %.6f" % got["q"][0])
    assert got["shell_n"][0].tolist() == [1] + [8] * 20 and got["valid"][0] and got["q"][0] > 0.99


def test_abi_has_the_entry_points():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native, ccp4, densityAnalysis as da, singleStructure
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdbeda.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("pdbeda_interp_density", "pdbeda_atom_qscores"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(handle, name) and re.search(r"\b%s\s*\(" % name, text)
    assert hasattr(_native.DeviceMap, "interp_density") and hasattr(_native.DeviceMap, "qscores")
    assert hasattr(ccp4.DensityMatrix, "getInterpolatedDensityFromXyz") and hasattr(ccp4.DensityMatrix, "qScores")
    assert "qscore" in singleStructure.MODES and all(("qscore", level) in singleStructure.TABLES for level in ("atom", "residue", "summary"))
    lead = da.DensityAnalysis.atomRegionDensityHeader[:6]
    assert da.DensityAnalysis.atomQScoreHeader == lead + ['bfactor', 'valid', 'q_score', 'n_points']
    assert da.DensityAnalysis.residueQScoreHeader == da.DensityAnalysis.residueRegionDensityHeader[:5] + ['mean_q_score', 'min_q_score', 'num_atoms_scored']
    source = open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_qscore.h")).read()
    assert int(re.search(r"QS_STAGE\s*=\s*(\d+)", source).group(1)) == qscore_cases.QS_STAGE
    assert "#define PDBEDA_QSCORE_MAX_LEVELS 8" in text and "#define PDBEDA_QSCORE_MAX_LEVEL_POINTS 64" in text


@pytest.mark.parametrize("name", qscore_cases.GOLDEN_MAPS)
def test_conditioning_of_the_gpu_cases(name):
    """The GPU tests compare q within 1e-9: the one-pass sums on the device lose about 1e-16 / ratio of a correlation, ratio = variance /
    mean square of an atom's sampled values, so the ratio must not be tiny for any atom that has a score (else: pick other seeds).  On
    skewed cells no kept point may lie on a face of a voxel either (there the checker's ``valid`` may not be the device's)."""
    z, header, grid = load_case(name)
    xyz = qscore_cases.chain(name, header)
    ref, unit, off = qscore_cases.tables()
    got = qscore_checker.qscores(header, grid, xyz, None, qscore_cases.STEP, ref, unit, off, qscore_cases.POINTS)
    have = np.isfinite(got["q"])
    print("%s: %d of %d atoms have a score, smallest variance / mean square %.3g, closest approach to a voxel face %.3g, most neighbours %d"
          % (name, int(have.sum()), len(xyz), float(np.nanmin(got["ratio"])), got["near_integer"], int(got["neighbours"].max())))
    assert have.sum() >= 200 and np.nanmin(got["ratio"]) >= 1e-4
    if not header.orthogonal:
        assert got["near_integer"] > 1e-9
