"""Blob shape descriptors without a GPU: tests/blobshape_checker.py on hand-made blobs whose answers are known on paper, the Python
finishing step (pdb_eda_amd.ccp4.blobShapeFinish) on skewed cells against the checker's direct computation, and the new entry point
declared, exported and bound."""
import ctypes
import io
import math
import re

import numpy as np
import pytest

from conftest import ROOT, load_case
import blobshape_checker as checker


def _header(spec, grid):
    from pdb_eda_amd import ccp4, synthetic
    header, _ = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, grid)))
    return header


def _orth(ncrs=(12, 10, 9), spacing=0.5, seed=5, **kw):
    """(header, grid) of a small orthogonal map, spacing exact in binary."""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=ncrs, spacing=spacing, **kw)
    grid = np.random.default_rng(seed).standard_normal((ncrs[2], ncrs[1], ncrs[0])).astype(np.float32)
    return _header(spec, grid), grid


def _moments(want):
    """The checker's sums in the shape of BlobList.moments()."""
    return {k: want[k] for k in ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2", "sw", "sw1", "sw2")}


def _finish(header, want, whole_map=False):
    from pdb_eda_amd import ccp4
    return ccp4.blobShapeFinish(header, want["n"], _moments(want), whole_map)


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_row_along_c(n):
    header, grid = _orth()
    crs = np.array([[c, 4, 3] for c in range(n)])
    want = checker.shape(header, grid, crs, [0, n])
    assert want["s1"].tolist() == [[n * (n - 1) // 2, 0, 0]]
    assert want["s2"].tolist() == [[(n - 1) * n * (2 * n - 1) // 6, 0, 0, 0, 0, 0]]
    var = 0.25 * (n * n - 1) / 12.0                                        # (n^2 - 1) / 12 voxels^2 at 0.5 A
    for got in (want, _finish(header, want)):
        assert np.allclose(got["secondMomentXyz"][0], np.diag([var, 0.0, 0.0]), rtol=0, atol=1e-12)
        assert np.allclose(got["principalLengths"][0], [math.sqrt(var), 0.0, 0.0], rtol=0, atol=1e-7)
        assert got["anisotropy"][0] == (1.0 if n > 1 else 0.0)
        assert np.allclose(got["boxExtent"][0], [0.5 * n, 0.5, 0.5], rtol=0, atol=1e-12)
    got = _finish(header, want)
    assert np.allclose(got["secondMomentCrs"][0], np.diag([(n * n - 1) / 12.0, 0.0, 0.0]), rtol=0, atol=1e-12)
    assert np.allclose(got["equivalentRadii"][0], math.sqrt(5.0) * got["principalLengths"][0])
    if n > 1:
        assert abs(abs(got["principalAxes"][0][0][0]) - 1.0) < 1e-12         # the long axis is x


def test_full_brick():
    header, grid = _orth()
    a, b, c = 3, 7, 5
    crs = np.array([[1 + i, 2 + j, 3 + k] for i in range(a) for j in range(b) for k in range(c)])
    want = checker.shape(header, grid, crs, [0, len(crs)])
    n = a * b * c
    assert want["boxLo"].tolist() == [[1, 2, 3]] and want["boxHi"].tolist() == [[a, b + 1, c + 2]]
    assert want["s1"].tolist() == [[n * (a - 1) // 2, n * (b - 1) // 2, n * (c - 1) // 2]]
    square = lambda m: (m - 1) * m * (2 * m - 1) // 6
    assert want["s2"][0, 0] == square(a) * b * c and want["s2"][0, 3] == square(b) * a * c and want["s2"][0, 5] == square(c) * a * b
    assert want["s2"][0, 1] == (a * (a - 1) // 2) * (b * (b - 1) // 2) * c
    var = sorted((0.25 * (m * m - 1) / 12.0 for m in (a, b, c)), reverse=True)
    for got in (want, _finish(header, want)):
        assert np.allclose(got["principalLengths"][0] ** 2, var, rtol=0, atol=1e-12)
        assert abs(got["anisotropy"][0] - (1.0 - math.sqrt(var[2] / var[0]))) < 1e-12
    assert np.allclose(_finish(header, want)["secondMomentCrs"][0], np.diag([(m * m - 1) / 12.0 for m in (a, b, c)]), rtol=0, atol=1e-12)


def test_plateau_extreme_is_first_in_crs_order():
    header, grid = _orth()
    grid[:] = 0.25
    grid[2:5, 3:6, 4:8] = -1.5                                               # grid is [s][r][c]: c 4..7, r 3..5, s 2..4
    crs = np.array([[c, r, s] for s in range(1, 6) for r in range(2, 7) for c in range(3, 9)])
    crs = crs[np.random.default_rng(3).permutation(len(crs))]               # the answer does not depend on the list's order
    want = checker.shape(header, grid, crs, [0, len(crs)])
    assert want["extremeCrs"].tolist() == [[4, 3, 2]] and want["extreme"][0] == np.float32(-1.5)
    assert np.array_equal(want["extremeXyz"][0], header.crs2xyz_array([[4, 3, 2]])[0])


def test_single_voxel():
    header, grid = _orth()
    want = checker.shape(header, grid, [[5, 6, 7]], [0, 1])
    assert not want["s1"].any() and not want["s2"].any() and not want["sw1"].any() and not want["sw2"].any()
    assert want["sw"][0] == abs(float(grid[7, 6, 5])) and want["extreme"][0] == grid[7, 6, 5]
    got = _finish(header, want)
    for k in ("secondMomentCrs", "secondMomentXyz", "principalLengths", "anisotropy", "weightedSecondMomentXyz", "weightedPrincipalLengths"):
        assert not np.any(got[k]), k
    assert np.allclose(got["weightedCentroid"][0], header.crs2xyz_array([[5, 6, 7]])[0], rtol=0, atol=1e-12)
    assert np.allclose(got["boxExtent"][0], [0.5, 0.5, 0.5]) and not got["onBorder"][0]


def test_raw_crs_outside_the_stored_grid():
    """8 x 8 x 8 stored voxels of a cell of 12 intervals: raw -1 wraps to 11, which is not stored (0); raw -5 wraps to 7, raw 13 to 1."""
    header, grid = _orth(ncrs=(8, 8, 8), interval=(12, 12, 12))
    crs = np.array([[-1, 0, 0], [-5, 0, 0], [13, 2, -12], [8, 0, 0], [3, -4, 20], [-13, -1, 0]])
    rho = checker.point_density(header, grid, crs)
    assert rho.tolist() == [0.0, float(grid[0, 0, 7]), float(grid[0, 2, 1]), 0.0, 0.0, 0.0]
    assert checker.point_density(header, grid, [[3, -5, 19]])[0] == float(grid[7, 7, 3])
    want = checker.shape(header, grid, crs, [0, 2, 6])
    assert want["boxLo"].tolist() == [[-5, 0, 0], [-13, -4, -12]] and want["boxHi"].tolist() == [[-1, 0, 0], [13, 2, 20]]
    assert want["extremeCrs"][0].tolist() == [-5, 0, 0] and want["s1"][0].tolist() == [4, 0, 0] and want["sw1"][0].tolist() == [0.0, 0.0, 0.0]
    assert want["extremeCrs"][1].tolist() == [13, 2, -12] and want["sw"][1] == abs(float(grid[0, 2, 1]))
    assert want["sw2"][1].tolist() == [abs(float(grid[0, 2, 1])) * x for x in (26 * 26, 26 * 6, 0, 36, 0, 0)]


@pytest.mark.parametrize("name", ["hex", "tric", "orth_perm"])
def test_finishing_on_skewed_and_permuted_cells(name):
    """blobShapeFinish (M C M^T from the integer sums) against the checker's sums over the voxels' xyz."""
    _, header, grid = load_case(name)
    rng = np.random.default_rng(17)
    blobs = [np.unique(rng.integers(-6, 15, size=(k, 3)) * [3, 1, 1], axis=0) for k in (1, 2, 7, 40, 300)]
    blobs.append(np.array([[c, 2 * c, 5] for c in range(9)]))                # a diagonal rod
    crs = np.concatenate(blobs)
    offsets = np.concatenate([[0], np.cumsum([len(b) for b in blobs])])
    want = checker.shape(header, grid, crs, offsets, whole_map=True)
    got = _finish(header, want, whole_map=True)
    tol = 1e-9 * want["boxDiagonal"] ** 2
    dense = want["sw"] > 0                                                   # (a blob of voxels that are not stored has no weighted moments: NaN on both sides)
    assert dense.sum() >= 4 and np.isfinite(want["secondMomentXyz"]).all()
    for k in ("weightedSecondMomentXyz", "weightedPrincipalLengths", "weightedCentroid"):
        assert np.isnan(got[k][~dense]).all() and np.isnan(want[k][~dense]).all(), k
    for k in ("secondMomentXyz", "weightedSecondMomentXyz"):
        keep = dense if k.startswith("weighted") else slice(None)
        assert np.all(np.abs(got[k] - want[k])[keep] <= tol[keep, None, None]), k
    for k in ("principalLengths", "weightedPrincipalLengths"):
        keep = dense if k.startswith("weighted") else slice(None)
        assert np.all(np.abs(got[k] ** 2 - want[k] ** 2)[keep] <= tol[keep, None]), k
    assert np.all(np.abs(got["weightedCentroid"] - want["weightedCentroid"])[dense] <= 1e-9 * want["boxDiagonal"][dense, None])
    assert np.all(np.abs(got["anisotropy"] - want["anisotropy"]) <= checker.anisotropy_bound(want, tol))
    assert np.allclose(got["boxExtent"], want["boxExtent"], rtol=1e-12, atol=0) and np.array_equal(got["extremeXyz"], want["extremeXyz"])
    assert np.array_equal(got["onBorder"], want["onBorder"]) and got["onBorder"].any()
    # the principal axes diagonalise the tensor they come from
    for b in range(len(blobs)):
        axes, cov = got["principalAxes"][b], got["secondMomentXyz"][b]
        assert np.allclose(axes.dot(cov).dot(axes.T), np.diag(got["principalLengths"][b] ** 2), rtol=0, atol=1e-9 * want["boxDiagonal"][b] ** 2)


def test_exact_numerator_beyond_int64():
    """n * sum d d' of a blob of 2^31 voxels and offsets near 2^15 leaves int64: the numerator is formed in Python integers."""
    from pdb_eda_amd import ccp4
    header, _ = _orth()
    n, d = 2 ** 31, 2 ** 15 - 1
    # half of the voxels at offset 0, half at d along c: variance d^2 / 4
    moments = {"boxLo": np.zeros((1, 3), np.int32), "boxHi": np.array([[d, 0, 0]], np.int32), "extremeCrs": np.zeros((1, 3), np.int32),
               "extreme": np.ones(1, np.float32), "s1": np.array([[n // 2 * d, 0, 0]], np.int64), "s2": np.array([[n // 2 * d * d, 0, 0, 0, 0, 0]], np.int64),
               "sw": np.array([float(n)]), "sw1": np.array([[n / 2 * d, 0.0, 0.0]]), "sw2": np.array([[n / 2 * d * d, 0, 0, 0, 0, 0.0]])}
    got = ccp4.blobShapeFinish(header, np.array([n], np.int64), moments)
    assert got["secondMomentCrs"][0, 0, 0] == d * d / 4.0 and got["weightedSecondMomentCrs"][0, 0, 0] == d * d / 4.0


def test_hand_made_blob_raises_a_clear_error():
    from pdb_eda_amd import ccp4
    blob = ccp4.DensityBlob([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1.0, 1.0, [[1, 2, 3]], None)
    assert blob.numVoxels == 1 and blob.atoms == []
    for name in ccp4.SHAPE_COLUMNS:
        with pytest.raises(AttributeError, match="device list"):
            getattr(blob, name)
    with pytest.raises(AttributeError):
        blob.anisotropy = 0.5                                                # read-only


def test_symbol_is_declared_exported_and_bound():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pdbeda.h").read(), flags=re.S)
    assert re.search(r"\bint\s+pdbeda_bloblist_moments\s*\(", text)
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "pdbeda_bloblist_moments")
    assert "pdbeda_bloblist_moments" in _native.EXPORTED_SYMBOLS and len(_native._SIGS["pdbeda_bloblist_moments"][1]) == 10
    assert len(_native.EXPORTED_SYMBOLS) >= 63
    assert callable(_native.BlobList.moments)


def test_shape_mode_is_listed():
    from pdb_eda_amd import densityAnalysis, singleStructure
    assert "shape" in singleStructure.MODES and ("shape", None) in singleStructure.TABLES
    header = singleStructure.TABLES[("shape", None)][0](None)
    assert header == densityAnalysis.DensityAnalysis.blobShapeHeader and len(header) == len(set(header)) == 21
