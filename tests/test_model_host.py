"""The model-density yardstick without a GPU: facts about tests/model_checker.py itself, the single-Gaussian atom model of ccp4.py, the
shift rule, the ABI of the two entry points, and the conditioning of every case tests/test_gpu_model.py runs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import model_cases
import model_checker


def test_one_atom_on_a_voxel_centre_gives_its_amplitude():
    header = model_cases.header_of("box")
    at = [10, 4, 3]
    xyz = np.array([header.crs2xyzCoord(at)], dtype=np.float64)
    got = model_checker.density(header, xyz, [[1.25]], [[2.0]], np.array([1.2], dtype=np.float32))
    assert got["exact"][at[2], at[1], at[0]] == 1.25 and got["count"][at[2], at[1], at[0]] == 1
    # 0.5 A beside it: exp(-2 * 0.25), one rounding each for the product inside and the product outside
    assert got["exact"][at[2], at[1], at[0] + 1] == 1.25 * np.exp(-(2.0 * 0.25))
    assert got["count"].sum() == (got["exact"] != 0).sum() and got["exact"].min() == 0.0 and not got["on_sphere"].any()


def test_two_identical_atoms_give_twice_one():
    header = model_cases.header_of("box")
    xyz, amp, expo, radii = model_cases.scattered("box", n=12)
    one = model_checker.density(header, xyz, amp, expo, radii)
    two = model_checker.density(header, np.concatenate([xyz, xyz]), np.concatenate([amp, amp]), np.concatenate([expo, expo]), np.concatenate([radii, radii]))
    assert np.array_equal(two["exact"], 2.0 * one["exact"]) and np.array_equal(two["count"], 2 * one["count"]) and one["count"].max() >= 2


def test_on_sphere_voxels_belong_to_the_sphere():
    header = model_cases.header_of("box")
    got = model_checker.density(header, *model_cases.on_sphere("box"))
    assert got["on_sphere"].sum() == 30 and np.all(got["exact"][got["on_sphere"]] == 0.75)          # (3, 0, 0) six times, (2, 2, 1) twenty-four times
    assert set(np.unique(got["exact"]).tolist()) == {0.0, 0.75}          # (expo = 0: a constant inside)


@pytest.mark.parametrize("n_sigma", [3.0, 4.0, 5.0])
def test_gaussian_atom_terms_integrate_to_occupancy_times_z(n_sigma):
    """One oxygen (Z = 8, occupancy 0.5, B = 30: sigma 0.62 A) in the middle of a 0.25 A grid: the sum over voxels times the voxel volume is
    occ * Z less the share beyond ``n_sigma`` sigmas, which the checker states in closed form.  The midpoint rule on a Gaussian of sigma /
    h = 2.5 is exact to far below 1e-6 (its error falls like exp(-2 pi^2 sigma^2 / h^2)); what remains is the ragged edge of the sphere on
    the grid, bounded by the shell of one voxel diagonal around it: 4 pi R^2 * (sqrt 3 h) * rho(R - sqrt 3 h)."""
    from pdb_eda_amd import ccp4, synthetic
    import io
    spec = synthetic.MapSpec(ncrs=(41, 41, 41), spacing=0.25)
    header = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((41, 41, 41), dtype=np.float32))))[0]
    amp, expo, b_eff = ccp4.gaussianAtomTerms([8.0], [30.0], [0.5])
    radii = ccp4.modelRadii(b_eff, n_sigma)
    assert b_eff[0] == 30.0 and radii.dtype == np.float32 and abs(float(radii[0]) - n_sigma * math.sqrt(30.0 / (8 * math.pi ** 2))) < 1e-6
    xyz = np.array([header.crs2xyzCoord([20, 20, 20])], dtype=np.float64) + [0.07, -0.04, 0.11]
    got = model_checker.density(header, xyz, amp, expo, radii, crs2xyz=header.crs2xyz_array, chunk=4096)
    found = math.fsum(got["exact"].reshape(-1).tolist()) * header.unitVolume
    want = 0.5 * 8.0 * (1.0 - model_checker.truncated_fraction(n_sigma))
    h, big_r = 0.25, float(radii[0])
    edge = 4 * math.pi * big_r ** 2 * (math.sqrt(3) * h) * float(amp[0]) * math.exp(-float(expo[0]) * (big_r - math.sqrt(3) * h) ** 2)
    print("nSigma %g: found %.6f, occ Z less the truncation %.6f, edge bound %.3g" % (n_sigma, found, want, edge))
    assert abs(found - want) <= edge + 1e-6 and found < 4.0


def test_atom_terms_floor_and_blur():
    from pdb_eda_amd import ccp4
    amp, expo, b_eff = ccp4.gaussianAtomTerms([6, 6, 6], [2.0, 20.0, 20.0], [1.0, 1.0, 0.0], blur=5.0)
    assert b_eff.tolist() == [ccp4.MODEL_MIN_B, 25.0, 25.0] and amp[2] == 0.0
    assert amp[1] == 6 * (4 * np.pi / 25.0) ** 1.5 and expo[1] == 4 * np.pi ** 2 / 25.0
    assert ccp4.modelRadii(b_eff)[1] == np.float32(ccp4.MODEL_N_SIGMA * np.sqrt(25.0 / (8 * np.pi ** 2)))


def test_shift_rule_at_its_edges():
    rule = model_checker.shift_rule
    assert rule(0, 5.0) == 40 and rule(100, 0.0) == 40 and rule(0, 0.0) == 40
    assert rule(1, 2.0 ** 22) == 40 and rule(1, np.nextafter(2.0 ** 22, np.inf)) == 39          # n A 2^40 <= 2^62 holds with equality, and just not
    assert rule(2 ** 20, 4.0) == 40 and rule(2 ** 20, 4.5) == 39 and rule(2 ** 20 + 1, 4.0) == 39
    assert rule(1, 2.0 ** 62) == 0 and rule(1, 2.0 ** 70) == -8 and rule(3, 1e-30) == 40
    assert model_checker.a_max(np.array([[1.0, -2.0], [0.5, 0.25]])) == 3.0 and model_checker.a_max(np.zeros((0, 1))) == 0.0


def test_pair_moments_of_the_checker():
    header = model_cases.header_of("rep")
    assert list(header.uniqueNcrs) == [16, 9, 7] and list(header.ncrs) == [21, 9, 7]
    a = np.arange(21 * 9 * 7, dtype=np.float32).reshape(7, 9, 21) % 5
    b = np.ones_like(a)
    b[:, :, 16:] = np.nan                                                # outside the unique box: never read
    n, sums, _ = model_checker.pair_moments(header, a, b)
    assert n == 16 * 9 * 7 and sums[1] == n and sums[3] == n and sums[0] == sums[4] == a[:, :, :16].sum()
    assert model_checker.pair_moments(header, a, b, floor=1.0)[0] == 0          # strict
    cc, scale, offset = model_checker.correlation(*model_checker.pair_moments(header, 2 * a + 1, a)[:2])
    assert abs(cc - 1) < 1e-12 and abs(scale - 2) < 1e-12 and abs(offset - 1) < 1e-12
    assert all(math.isnan(v) for v in model_checker.correlation(*model_checker.pair_moments(header, a, b)[:2])[:2])


def test_abi_has_the_entry_points():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native, ccp4, densityAnalysis as da, singleStructure
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdbeda.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("pdbeda_model_density", "pdbeda_map_pair_moments"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(handle, name) and re.search(r"\b%s\s*\(" % name, text)
    assert hasattr(_native.DeviceMap, "model_density") and hasattr(_native.DeviceMap, "pair_moments")
    assert all(hasattr(ccp4.DensityMatrix, name) for name in ("modelDensity", "pairMoments", "correlate"))
    assert all(hasattr(da.DensityAnalysis, name) for name in ("modelDensityObj", "modelCorrelation", "modelDifferenceObj", "calculateAtomModelCorrelations",
                                                               "calculateResidueModelCorrelations", "modelSummary"))
    assert "model" in singleStructure.MODES and all(("model", level) in singleStructure.TABLES for level in ("atom", "residue", "summary"))
    assert da.DensityAnalysis.atomModelCorrelationHeader == da.DensityAnalysis.atomRegionDensityHeader[:6] + ['bfactor', 'rscc_model', 'rsr_model']
    assert da.DensityAnalysis.residueModelCorrelationHeader == da.DensityAnalysis.residueRegionDensityHeader[:5] + ['rscc_model', 'rsr_model']
    assert da.modelBlur == 0.0 and da.modelSigmas == ccp4.MODEL_N_SIGMA
    source = open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_model.h")).read()
    assert int(re.search(r"MD_STAGE\s*=\s*(\d+)", source).group(1)) == model_cases.STAGE
    tile = re.search(r"PT_C\s*=\s*(\d+),\s*PT_R\s*=\s*(\d+),\s*PT_S\s*=\s*(\d+)", open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_partition.h")).read())
    assert tuple(int(v) for v in tile.groups()) == model_cases.TILE
    assert "#define PDBEDA_MODEL_MAX_TERMS 6" in text


@pytest.mark.parametrize("tag,name,atoms", model_cases.conditioned_cases(), ids=[c[0] for c in model_cases.conditioned_cases()])
def test_conditioning_of_the_gpu_cases(tag, name, atoms):
    """No pair within 1e-9 of its sphere (membership must not hinge on an ulp of crs2xyz or of the distance), every non-zero term at least
    2^-14 (tests/model_cases.py says why), and the case is not vacuous."""
    header = model_cases.header_of(name)
    got = model_checker.density(header, *atoms)
    print("%s: nearest approach to a sphere %.3g, smallest term %.3g, most atoms on a voxel %d, reached voxels %d of %d"
          % (tag, got["nearest_sphere"], got["smallest_term"], int(got["count"].max()), int((got["count"] > 0).sum()), got["count"].size))
    assert not got["on_sphere"].any() and got["nearest_sphere"] > 1e-9
    assert got["smallest_term"] >= 2.0 ** -14
    assert (got["count"] > 0).any() and got["count"].max() >= 2
    if not tag.startswith("clustered"):
        assert (got["count"] == 0).any()          # (unreached voxels: exact zeros to check)
