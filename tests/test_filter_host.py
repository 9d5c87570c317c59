"""The filter tests' own foundations, without a GPU: tests/filter_checker.py (the restatement the device is held to, bit for bit, in
tests/test_gpu_filter.py) against scipy.ndimage and against direct windowed numpy statistics, the tap helpers, and the new surface.

The bound against scipy, 1e-12 max|x|: both sides add 2R + 1 products per axis in fp64, in different orders; 3 (2R + 1) roundings of
1.1e-16 relative to sums of positive weights that add up to 1 stay below 3 * 49 * 1.1e-16 = 1.6e-14 at R = 24.  Observed: 1.1e-16 to
2.8e-16 on an 11 x 13 x 19 box at radii up to 24."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT
import filter_cases
import filter_checker

from pdb_eda_amd import ccp4


def _close(got, want, x, what):
    err = float(np.max(np.abs(got - want)))
    bound = 1e-12 * float(np.max(np.abs(x)))
    print("%s: max |checker - scipy| = %.3g (bound %.3g)" % (what, err, bound))
    assert err <= bound, what


def _gauss(x, sigmas_crs, intervals, truncate=4.0):
    taps = [ccp4.gaussianTaps(s, truncate) for s in sigmas_crs]
    return filter_checker.filter3(x, taps, intervals), taps


def test_gaussian_taps_are_scipys():
    for sigma, truncate in ((1.5, 4.0), (0.8, 4.0), (6.0, 4.0), (2.5, 3.0), (16.0, 4.0)):
        w = ccp4.gaussianTaps(sigma, truncate)
        radius = int(truncate * sigma + 0.5)
        assert len(w) == 2 * radius + 1
        delta = np.zeros(2 * radius + 1)
        delta[radius] = 1.0
        want = ndimage.gaussian_filter1d(delta, sigma, truncate=truncate, mode="constant")
        assert np.max(np.abs(w - want)) <= 1e-16 and abs(w.sum() - 1.0) <= 1e-15
    assert ccp4.gaussianTaps(0.0).tolist() == [1.0] and ccp4.gaussianTaps(0.1).tolist() == [1.0]
    assert ccp4.boxTaps(0).tolist() == [1.0] and ccp4.boxTaps(3).tolist() == [1.0 / 7] * 7
    with pytest.raises(ValueError):
        ccp4.gaussianTaps(-1.0)
    with pytest.raises(ValueError):
        ccp4.gaussianTaps(float("nan"))
    with pytest.raises(ValueError):
        ccp4.boxTaps(-1)


def test_checker_wraps_like_scipy_on_a_full_cell():
    x = filter_cases.grid_of("box").astype(np.float64)
    got, _ = _gauss(x, (1.5, 0.8, 0.4), filter_cases.intervals_of("box"))
    _close(got, ndimage.gaussian_filter(x, sigma=(0.4, 0.8, 1.5), mode="wrap"), x, "box, radii 6 / 3 / 2")


def test_checker_wraps_radii_larger_than_the_axis():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((19, 13, 11)) + 2.0
    got, taps = _gauss(x, (3.0, 4.0, 6.0), (11, 13, 19))
    assert [len(t) // 2 for t in taps] == [12, 16, 24]          # each beyond its axis of 11, 13, 19
    _close(got, ndimage.gaussian_filter(x, sigma=(6.0, 4.0, 3.0), mode="wrap"), x, "11 x 13 x 19, radii 12 / 16 / 24")
    x = filter_cases.grid_of("box").astype(np.float64)
    got, _ = _gauss(x, (6.0, 3.0, 3.0), filter_cases.intervals_of("box"))
    _close(got, ndimage.gaussian_filter(x, sigma=(3.0, 3.0, 6.0), mode="wrap"), x, "box, radii 24 / 12 / 12")


def test_checker_sees_zeros_outside_a_cut_out():
    x = filter_cases.grid_of("skew").astype(np.float64)
    iv = filter_cases.intervals_of("skew")
    assert iv == [32, 16, 12] and all(i - n >= r for i, n, r in zip(iv, (21, 9, 7), (6, 3, 2)))          # the halo never wraps into the stored box
    got, _ = _gauss(x, (1.5, 0.8, 0.4), iv)
    _close(got, ndimage.gaussian_filter(x, sigma=(0.4, 0.8, 1.5), mode="constant", cval=0.0), x, "skew cut-out")


def test_checker_reads_the_copies_of_a_repeating_box():
    """rep stores 21 columns of a 16-column cell: a neighbour outside the box is column j mod 16, never absent."""
    idx = filter_checker.source_index(21, 16, 3)
    assert idx.min() >= 0 and idx[0].tolist() == [13, 14, 15, 0, 1, 2, 3] and idx[20].tolist() == [17, 18, 19, 20, 5, 6, 7]
    cut = filter_checker.source_index(21, 32, 3)
    assert cut[0].tolist() == [-1, -1, -1, 0, 1, 2, 3] and cut[20].tolist() == [17, 18, 19, 20, -1, -1, -1]
    far = filter_checker.source_index(5, 8, 9)                  # wraps more than once
    assert far[0].tolist() == [-1, 0, 1, 2, 3, 4, -1, -1, -1, 0, 1, 2, 3, 4, -1, -1, -1, 0, 1]


def test_box_taps_are_the_uniform_filter():
    x = filter_cases.grid_of("box").astype(np.float64)
    taps = (ccp4.boxTaps(2), ccp4.boxTaps(1), ccp4.boxTaps(3))
    got = filter_checker.filter3(x, taps, filter_cases.intervals_of("box"))
    _close(got, ndimage.uniform_filter(x, size=(7, 3, 5), mode="wrap"), x, "box taps")


@pytest.mark.parametrize("name", ["box", "skew", "rep", "cut"])
@pytest.mark.parametrize("taps", ["gauss", "one_sided"])
def test_weights_are_the_filter_of_ones(name, taps):
    t = filter_cases.tap_sets()[taps]
    iv = filter_cases.intervals_of(name)
    shape = filter_cases.grid_of(name).shape
    n = filter_checker.norm3(shape, t, iv)
    ones = filter_checker.filter3(np.ones(shape), t, iv)
    assert np.max(np.abs(n - ones)) <= 1e-15
    if taps == "one_sided" and name in ("skew", "cut"):
        assert (n == 0).any() and (n > 0).any()                 # the high faces of a cut-out meet nothing
    else:
        assert (n > 0).all()
    if name in ("box", "rep") and taps == "gauss":
        assert np.max(np.abs(n - 1.0)) <= 1e-15                 # periodic: every tap meets a voxel


def test_renormalised_filter_keeps_a_constant():
    c = np.full(filter_cases.grid_of("skew").shape, 2.5, dtype=np.float32)
    t = filter_cases.tap_sets()["gauss"]
    iv = filter_cases.intervals_of("skew")
    plain = filter_checker.map_filter(c, t, iv)
    mean = filter_checker.map_filter(c, t, iv, renormalize=True)
    assert plain.dtype == mean.dtype == np.float32
    assert plain.min() < 2.0 and np.max(np.abs(mean - 2.5)) <= 1e-6


def test_local_formulas_against_direct_windows():
    """Mean, standard deviation, z and correlation of a periodic box window against np.mean / np.std / np.corrcoef over the same voxels."""
    a = filter_cases.grid_of("box")
    b = filter_cases.grid_of("box", seed=1, offset=-0.5)
    h = (2, 1, 1)                                               # half widths along c, r, s
    taps = [ccp4.boxTaps(v) for v in h]
    got = filter_checker.local_stats(a, b, taps, filter_cases.intervals_of("box"))
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for s, r, c in ((0, 0, 0), (3, 4, 10), (6, 8, 20), (2, 0, 19), (5, 7, 1)):
        idx = np.ix_(np.arange(s - h[2], s + h[2] + 1) % 7, np.arange(r - h[1], r + h[1] + 1) % 9, np.arange(c - h[0], c + h[0] + 1) % 21)
        wa, wb = a64[idx].reshape(-1), b64[idx].reshape(-1)
        assert abs(got["mean_a"][s, r, c] - wa.mean()) <= 1e-6 and abs(got["std_b"][s, r, c] - wb.std()) <= 1e-6      # (float32 outputs)
    # the same in fp64, before the outputs are rounded
    iv = filter_cases.intervals_of("box")
    ea, eaa = filter_checker.filter3(a64, taps, iv), filter_checker.filter3(a64 * a64, taps, iv)
    eb, ebb, eab = filter_checker.filter3(b64, taps, iv), filter_checker.filter3(b64 * b64, taps, iv), filter_checker.filter3(a64 * b64, taps, iv)
    for s, r, c in ((0, 0, 0), (3, 4, 10), (6, 8, 20), (2, 0, 19), (5, 7, 1)):
        idx = np.ix_(np.arange(s - h[2], s + h[2] + 1) % 7, np.arange(r - h[1], r + h[1] + 1) % 9, np.arange(c - h[0], c + h[0] + 1) % 21)
        wa, wb = a64[idx].reshape(-1), b64[idx].reshape(-1)
        at = (s, r, c)
        va, vb = eaa[at] - ea[at] ** 2, ebb[at] - eb[at] ** 2
        assert abs(ea[at] - wa.mean()) <= 1e-9 and abs(np.sqrt(va) - wa.std()) <= 1e-9 and abs(np.sqrt(vb) - wb.std()) <= 1e-9
        assert abs((eab[at] - ea[at] * eb[at]) / np.sqrt(va * vb) - np.corrcoef(wa, wb)[0, 1]) <= 1e-9
        assert abs(got["z_a"][at] - (a64[at] - wa.mean()) / wa.std()) <= 1e-5 and abs(got["cc"][at] - np.corrcoef(wa, wb)[0, 1]) <= 1e-6


def test_local_stats_edge_rules():
    a = filter_cases.grid_of("skew")
    iv = filter_cases.intervals_of("skew")
    const = np.full(a.shape, 3.0, dtype=np.float32)
    t = filter_cases.tap_sets()["box"]
    out = filter_checker.local_stats(const, a, t, iv)
    assert np.all(out["std_a"] <= 1e-6) and np.all(out["cc"][out["std_a"] == 0] == 0)
    floor = filter_checker.local_stats(const, None, t, iv, std_floor=0.5)
    assert np.all(np.abs(floor["z_a"]) <= 1e-6)
    lin = filter_checker.local_stats(a, (2.0 * a.astype(np.float64) + 1.0).astype(np.float32), t, iv)
    assert np.all(lin["cc"] >= 0.999)
    t0 = filter_cases.tap_sets()["one_sided"]
    empty = filter_checker.norm3(a.shape, t0, iv) == 0
    out = filter_checker.local_stats(a, a, t0, iv)
    assert empty.any() and all(np.all(v[empty] == 0) for v in out.values())


def test_new_symbols_and_modes():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native, singleStructure
    text = open(os.path.join(ROOT, "include", "pdbeda.h")).read()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("pdbeda_map_filter", "pdbeda_map_local_stats"):
        assert re.search(r"\bint %s\s*\(" % name, text) and hasattr(handle, name) and name in _native.EXPORTED_SYMBOLS
    assert re.search(r"#define PDBEDA_FILTER_MAX_RADIUS\s+64\b", text) and re.search(r"#define PDBEDA_FILTER_RENORMALIZE\s+1u\b", text)
    assert _native.FILTER_MAX_RADIUS == ccp4.FILTER_MAX_RADIUS == filter_cases.MAX_RADIUS == 64 and _native.FILTER_RENORMALIZE == 1
    kernels = open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_filter.h")).read()
    for name, value in (("FC_RUN", filter_cases.UNIT_C[0]), ("FC_ROWS", filter_cases.UNIT_C[1]), ("FL_LANES", filter_cases.UNIT_LINE[0]), ("FL_CHUNK", filter_cases.UNIT_LINE[1])):
        assert re.search(r"constexpr int %s = %d;" % (name, value), kernels), name
    assert "local" in singleStructure.MODES
    assert all(("local", level) in singleStructure.TABLES for level in ("atom", "residue", "summary"))


def _hostOnly(name):
    """A DensityMatrix with a header and no device: enough for the argument checks that come before any call."""
    return ccp4.DensityMatrix.fromDeviceMap(filter_cases.header_of(name), None, None, name, None)


def test_gaussian_filter_refuses_before_the_device():
    skew = _hostOnly("skew")
    with pytest.raises(ValueError, match="voxels=True"):
        skew.gaussianFilter(1.0)
    with pytest.raises(ValueError, match="voxels=True"):
        skew.localStats(sigma=1.0)
    box = _hostOnly("box")
    with pytest.raises(ValueError, match="radius 66"):          # 0.5 A steps: 8.2 A = 16.4 steps, int(65.6 + 0.5) = 66
        box.gaussianFilter(8.2)
    with pytest.raises(ValueError, match="radius 65"):
        box.gaussianFilter(16.2, voxels=True)                   # int(64.8 + 0.5)
    with pytest.raises(ValueError):
        box.localStats()
    with pytest.raises(ValueError):
        box.localStats(taps=ccp4.boxTaps(1), sigma=1.0)
    assert [len(t) // 2 for t in box._gaussianTapsPerAxis(0.75, 4.0, False)] == [6, 6, 6]
    assert [len(t) // 2 for t in skew._gaussianTapsPerAxis(16.0, 4.0, True)] == [64, 64, 64]
