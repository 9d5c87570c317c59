"""The peak-search contract without a GPU: the numpy checker (tests/peaks_checker.py, the yardstick of tests/test_gpu_peaks.py)
on hand-made grids whose answer is written out here, and the six new names of the C-ABI in the header, the built library and
the ctypes stub."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
import peaks_checker

PEAK_SYMBOLS = ["pdbeda_map_peaks", "pdbeda_map_peaks_pm", "pdbeda_peaklist_count", "pdbeda_peaklist_counters", "pdbeda_peaklist_free",
                "pdbeda_peaklist_rows"]


def _header(ncrs, **kw):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(synthetic.MapSpec(ncrs=ncrs, spacing=0.5, **kw)))


def _grid(ncrs, fill=0.0):
    nc, nr, ns = ncrs
    return np.full((ns, nr, nc), fill, dtype=np.float32)      # stored [s][r][c]


def _put(grid, crs, value):
    grid[crs[2], crs[1], crs[0]] = value


def test_one_interior_maximum():
    ncrs = (7, 6, 5)
    h, g = _header(ncrs), _grid(ncrs)
    _put(g, (3, 2, 2), 4.0)
    _put(g, (2, 2, 2), 1.0)       # c - 1
    _put(g, (4, 2, 2), 2.0)       # c + 1
    _put(g, (3, 1, 2), 3.0)       # r - 1
    _put(g, (3, 3, 2), 3.0)       # r + 1: symmetric, offset 0
    got = peaks_checker.find_peaks(h, g, 3.5)
    assert got["crs"].tolist() == [[3, 2, 2]] and got["height"].tolist() == [4.0] and got["on_border"].tolist() == [False]
    # c axis: a = 1, v = 4, b = 2: den = -5, offset = 0.5 * (1 - 2) / -5 = 0.1;  s axis: a = b = 0: offset 0
    assert np.allclose(got["offset"], [[0.1, 0.0, 0.0]], rtol=0, atol=1e-15)
    assert got["refined_height"][0] == 4.0 - 0.25 * ((1.0 - 2.0) * got["offset"][0, 0])
    assert np.allclose(got["refined_xyz"], [[3.1 * 0.5, 2 * 0.5, 2 * 0.5]], rtol=0, atol=1e-6)     # (float32 cell lengths in the header)
    # the same voxel is no peak of the negative side, and nothing passes a cutoff above it
    assert len(peaks_checker.find_peaks(h, g, -3.5)["crs"]) == 0
    assert len(peaks_checker.find_peaks(h, g, 4.5)["crs"]) == 0


def test_plateau_has_exactly_one_peak_its_c_major_first_voxel():
    ncrs = (6, 6, 6)
    h, g = _header(ncrs), _grid(ncrs)
    for c in (2, 3):
        for r in (2, 3):
            for s in (3, 4):
                _put(g, (c, r, s), 2.0)
    got = peaks_checker.find_peaks(h, g, 1.0)
    assert got["crs"].tolist() == [[2, 2, 3]]


def test_two_equal_maxima_come_in_c_major_order():
    ncrs = (9, 5, 5)
    h, g = _header(ncrs), _grid(ncrs)
    _put(g, (6, 1, 3), 5.0)
    _put(g, (2, 3, 1), 5.0)
    _put(g, (4, 2, 2), 7.0)
    got = peaks_checker.find_peaks(h, g, 1.0)
    assert got["crs"].tolist() == [[4, 2, 2], [2, 3, 1], [6, 1, 3]]          # height first, then (c, r, s)
    assert got["key"][1] < got["key"][2]


def test_corner_maximum_is_on_the_border_with_clipped_axes():
    ncrs = (5, 5, 5)
    h, g = _header(ncrs), _grid(ncrs)
    _put(g, (0, 0, 2), 3.0)
    _put(g, (1, 0, 2), 2.0)
    _put(g, (0, 1, 2), 2.0)
    _put(g, (0, 0, 1), 1.0)
    _put(g, (0, 0, 3), 2.0)
    got = peaks_checker.find_peaks(h, g, 2.5)
    assert got["crs"].tolist() == [[0, 0, 2]] and got["on_border"].tolist() == [True]
    # c and r are clipped (offset 0); s: a = 1, v = 3, b = 2: den = -3, offset = 0.5 * -1 / -3
    assert got["offset"][0, 0] == 0.0 and got["offset"][0, 1] == 0.0 and got["offset"][0, 2] == (0.5 * (1.0 - 2.0)) / ((1.0 - 6.0) + 2.0)
    assert got["refined_height"][0] == 3.0 - 0.25 * ((1.0 - 2.0) * got["offset"][0, 2])


def test_minimum_with_negative_cutoff():
    ncrs = (6, 5, 7)
    h, g = _header(ncrs), _grid(ncrs)
    _put(g, (3, 2, 4), -4.0)
    _put(g, (3, 2, 3), -1.0)
    _put(g, (1, 1, 1), 9.0)
    got = peaks_checker.find_peaks(h, g, -2.0)
    assert got["crs"].tolist() == [[3, 2, 4]] and got["height"].tolist() == [-4.0]
    # s axis: a = -1, v = -4, b = 0: den = 7, offset = 0.5 * -1 / 7
    assert got["offset"][0].tolist() == [0.0, 0.0, (0.5 * (-1.0 - 0.0)) / 7.0]
    assert got["refined_height"][0] == -4.0 - 0.25 * ((-1.0 - 0.0) * got["offset"][0, 2]) and got["refined_height"][0] < -4.0


def test_value_equal_to_the_cutoff_is_kept():
    ncrs = (5, 5, 5)
    h, g = _header(ncrs), _grid(ncrs)
    cut = 1.1                                  # float32(1.1) is the cutoff the library sees
    _put(g, (2, 2, 2), np.float32(cut))
    _put(g, (4, 4, 4), np.nextafter(np.float32(cut), np.float32(0)))
    got = peaks_checker.find_peaks(h, g, cut)
    assert got["crs"].tolist() == [[2, 2, 2]]


def test_domain_is_clipped_to_unique_ncrs():
    ncrs = (8, 5, 5)
    h = _header(ncrs, interval=(6, 5, 5))      # 8 columns stored, the cell repeats after 6
    assert list(h.uniqueNcrs) == [6, 5, 5]
    g = _grid(ncrs)
    _put(g, (7, 2, 2), 9.0)                    # outside the unique box: neither a peak nor a neighbour
    _put(g, (5, 2, 2), 3.0)                    # last unique column; its stored neighbour at c = 6 is higher, and is not looked at
    _put(g, (6, 2, 2), 5.0)
    got = peaks_checker.find_peaks(h, g, 1.0)
    assert got["crs"].tolist() == [[5, 2, 2]] and got["on_border"].tolist() == [True]
    assert got["offset"][0, 0] == 0.0


def test_nan_voxel_is_never_a_peak_and_beats_nothing():
    ncrs = (5, 5, 5)
    h, g = _header(ncrs), _grid(ncrs)
    _put(g, (2, 2, 2), np.nan)
    _put(g, (1, 2, 2), 3.0)                    # a neighbour of the NaN: it does not beat it
    _put(g, (4, 0, 0), 2.0)
    got = peaks_checker.find_peaks(h, g, 1.0)
    assert got["crs"].tolist() == [[4, 0, 0]]


def test_peak_symbols_are_declared_exported_and_bound():
    """Fails on a tree without the feature: the six names are in include/pdbeda.h, in the built library and in the stub."""
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdbeda.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pdbeda_[a-z0-9_]+)\s*\(", text))
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in PEAK_SYMBOLS:
        assert name in declared, name
        assert hasattr(handle, name), name
        assert name in _native.EXPORTED_SYMBOLS, name
