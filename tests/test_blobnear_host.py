"""Nearest-blob search without a GPU: tests/blobnear_checker.py on hand-made grids whose answers are known on paper, the neighbourhood
table (pdb_eda_amd.ccp4.neighbourOffsets) on orthogonal, hexagonal and triclinic headers, the dipole columns from canned inputs, and the
new entry point declared, exported and bound."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT, load_case
import blobnear_checker as checker

BOX26 = [(dc, dr, ds) for dc in (-1, 0, 1) for dr in (-1, 0, 1) for ds in (-1, 0, 1) if (dc, dr, ds) != (0, 0, 0)]


def _volume(shape, blobs):
    """blobs: a list of lists of (c, r, s) -> the label volume [s][r][c]."""
    lab = np.full(shape, -1, dtype=np.int64)
    for i, voxels in enumerate(blobs):
        for c, r, s in voxels:
            lab[s, r, c] = i
    return lab


def test_two_voxels():
    shape = (5, 6, 7)                                                        # ns, nr, nc
    a, b = _volume(shape, [[(2, 3, 1)]]), _volume(shape, [[(6, 0, 0)], [(3, 3, 1)]])
    table = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0)]
    got = checker.nearest(a, b, table, 1)
    assert got["index"].tolist() == [2] and got["partner"].tolist() == [1]
    assert got["voxel"].tolist() == [[2, 3, 1]] and got["partnerVoxel"].tolist() == [[3, 3, 1]]
    back = checker.nearest(b, a, table, 2)                                   # the other way: blob 1 reaches it by (-1, 0, 0), blob 0 does not
    assert back["index"].tolist() == [-1, 1] and back["partner"].tolist() == [-1, 0]
    assert back["voxel"].tolist() == [[0, 0, 0], [3, 3, 1]] and back["partnerVoxel"].tolist() == [[0, 0, 0], [2, 3, 1]]
    # a table that does not hold the offset: no pair; an empty table: no pair
    assert checker.nearest(a, b, [(0, 0, 1), (0, 0, -1)], 1)["index"].tolist() == [-1]
    assert checker.nearest(a, b, np.zeros((0, 3), int), 1)["partner"].tolist() == [-1]


def test_tie_goes_to_the_offset_order_then_to_the_position():
    shape = (6, 6, 8)
    # blob 0 of a: two voxels; (1, 2, 2) has b on its +c side, (5, 2, 2) on its -c side: both at one step
    a = _volume(shape, [[(1, 2, 2), (5, 2, 2)]])
    b = _volume(shape, [[(2, 2, 2)], [(4, 2, 2)]])
    got = checker.nearest(a, b, [(-1, 0, 0), (1, 0, 0)], 1)                  # (-1, 0, 0) comes first in the table: the voxel at c = 5 wins
    assert got["index"].tolist() == [0] and got["voxel"].tolist() == [[5, 2, 2]] and got["partner"].tolist() == [1]
    got = checker.nearest(a, b, [(1, 0, 0), (-1, 0, 0)], 1)                  # the table the other way round: the other voxel
    assert got["index"].tolist() == [0] and got["voxel"].tolist() == [[1, 2, 2]] and got["partner"].tolist() == [0]
    # the same t for several voxels: the first in (c, r, s) order, c most significant
    a = _volume(shape, [[(3, 4, 1), (3, 1, 5), (2, 5, 5), (3, 1, 2)]])
    b = _volume(shape, [[(3, 4, 2), (3, 1, 4), (2, 5, 4), (3, 1, 3)]])
    got = checker.nearest(a, b, [(0, 0, 1), (0, 0, -1)], 1)
    assert got["index"].tolist() == [0] and got["voxel"].tolist() == [[3, 1, 2]] and got["partnerVoxel"].tolist() == [[3, 1, 3]]
    got = checker.nearest(a, b, [(0, 0, -1), (0, 0, 1)], 1)
    assert got["index"].tolist() == [0] and got["voxel"].tolist() == [[2, 5, 5]] and got["partnerVoxel"].tolist() == [[2, 5, 4]]


def test_nothing_wraps():
    shape = (4, 4, 6)
    a, b = _volume(shape, [[(0, 1, 1)]]), _volume(shape, [[(5, 1, 1)]])       # c = 0 and c = nc - 1: neighbours only through the wrap
    assert checker.nearest(a, b, BOX26, 1)["index"].tolist() == [-1]
    assert checker.nearest(b, a, BOX26, 1)["index"].tolist() == [-1]
    assert checker.nearest(a, b, BOX26 + [(5, 0, 0)], 1)["index"].tolist() == [26]          # ... but five steps along c inside the box
    assert checker.nearest(a, b, [(6, 0, 0), (-6, 0, 0), (-1, 0, 0)], 1)["index"].tolist() == [-1]          # offsets wider than the box


def test_overlap_of_two_maps_is_the_zero_offset():
    shape = (3, 3, 3)
    a, b = _volume(shape, [[(0, 0, 0), (1, 1, 1)], [(2, 2, 2)]]), _volume(shape, [[(2, 0, 0)], [(1, 1, 1)]])
    got = checker.nearest(a, b, [(0, 0, 0)] + BOX26, 2)
    assert got["index"].tolist() == [0, 1 + BOX26.index((-1, -1, -1))] and got["partner"].tolist() == [1, 1]
    assert got["voxel"].tolist() == [[1, 1, 1], [2, 2, 2]]


def _direct(header, offsets):
    return np.array([np.linalg.norm(np.asarray(header.crs2xyzCoord(list(o)), dtype=np.float64) - np.asarray(header.crs2xyzCoord([0, 0, 0]), dtype=np.float64))
                     for o in offsets.tolist()])


@pytest.mark.parametrize("name", ["orth", "orth_perm", "hex", "tric"])
@pytest.mark.parametrize("reach", [0.0, 1.5, 2.5])
def test_neighbour_offsets(name, reach):
    from pdb_eda_amd import ccp4
    _, header, _ = load_case(name)
    offsets, distance = ccp4.neighbourOffsets(header, reach)
    assert offsets.dtype == np.int32 and offsets.shape == (len(distance), 3) and distance.dtype == np.float64
    assert offsets[0].tolist() == [0, 0, 0] and distance[0] == 0.0
    direct = _direct(header, offsets)
    assert np.allclose(distance, direct, rtol=0, atol=1e-9) and (distance <= reach).all()
    # sorted: ascending squared length, ties by (dc, dr, ds)
    step = header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3)))
    d2 = np.einsum("ni,ij,nj->n", offsets.astype(np.float64), step.dot(step.T), offsets.astype(np.float64))
    keys = list(zip(d2.tolist(), *offsets.T.tolist()))
    assert keys == sorted(keys) and len(set(map(tuple, offsets.tolist()))) == len(offsets)
    # symmetric under o -> -o
    assert set(map(tuple, offsets.tolist())) == set(map(tuple, (-offsets).tolist()))
    # complete: every offset of a box that holds the ball, computed the direct way (1e-9 A either side of the rim is nobody's)
    n = int(np.abs(offsets).max()) + 2
    every = np.array([(c, r, s) for c in range(-n, n + 1) for r in range(-n, n + 1) for s in range(-n, n + 1)], dtype=np.int32)
    inside = _direct(header, every)
    assert (inside.reshape(2 * n + 1, 2 * n + 1, 2 * n + 1)[[0, -1]] > reach).all()          # (the box does hold it)
    assert {tuple(o) for o in every[inside <= reach - 1e-9].tolist()} <= set(map(tuple, offsets.tolist()))
    assert len(offsets) <= int((inside <= reach + 1e-9).sum())
    if reach > 0:
        assert len(offsets) >= 27


def test_neighbour_offsets_limits():
    from pdb_eda_amd import ccp4
    _, header, _ = load_case("orth")
    step = float(min(np.linalg.norm(header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3))), axis=1)))
    # a ball of radius R voxels holds about 4.19 R^3 offsets: 16384 are passed near R = 15.8, +-127 far later
    assert len(ccp4.neighbourOffsets(header, 10.0 * step)[0]) <= ccp4.NEAREST_MAX_OFFSETS
    for reach in (20.0 * step, 130.0 * step, 1e6):
        with pytest.raises(ValueError):
            ccp4.neighbourOffsets(header, reach)
    with pytest.raises(ValueError):
        ccp4.neighbourOffsets(header, -1.0)
    with pytest.raises(ValueError):
        ccp4.neighbourOffsets(header, float("nan"))
    with pytest.raises(ValueError, match="finite"):
        ccp4.neighbourOffsets(header, float("inf"))
    assert ccp4.NEAREST_MAX_OFFSETS == 16384 and ccp4.NEAREST_MAX_COMPONENT == 127


def test_dipole_columns_from_canned_inputs():
    from pdb_eda_amd import densityAnalysis
    nan = float("nan")
    near = {"partner": np.array([1, -1, 0], np.int32), "distance": np.array([1.0, nan, 2.0]),
            "voxelXyz": np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [4.0, 0.0, 0.0]]), "partnerVoxelXyz": np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [4.0, 2.0, 0.0]])}
    back = {"partner": np.array([0, 0], np.int32)}                           # both red blobs name green 0: the pair (2, 0) is not mutual
    d = densityAnalysis.blobDipoleColumns(near, back, greenTotal=[4.0, 9.0, 1.0], redTotal=[-8.0, -2.0], greenCentroid=[[0, 0, 0], [9, 9, 9], [4, 0, 0]],
                                          redCentroid=[[4, 3, 0], [3, 0, 0]], ratio=2.0)
    assert d["green"].tolist() == [0, 2] and d["red"].tolist() == [1, 0] and d["gap"].tolist() == [1.0, 2.0] and d["mutual"].tolist() == [True, False]
    assert d["greenElectrons"].tolist() == [2.0, 0.5] and d["redElectrons"].tolist() == [1.0, 4.0] and d["balance"].tolist() == [0.5, 0.125]
    assert d["centroidDistance"].tolist() == [3.0, 3.0] and d["shift"].tolist() == [[-3.0, 0.0, 0.0], [0.0, -3.0, 0.0]]
    assert d["midpoint"].tolist() == [[0.5, 0.0, 0.0], [4.0, 1.0, 0.0]]
    # no pair at all: no row
    none = densityAnalysis.blobDipoleColumns({"partner": np.array([-1, -1]), "distance": np.array([nan, nan]), "voxelXyz": np.zeros((2, 3)), "partnerVoxelXyz": np.zeros((2, 3))},
                                             {"partner": np.array([-1])}, [1.0, 1.0], [-1.0], np.zeros((2, 3)), np.zeros((1, 3)), 2.0)
    assert all(len(v) == 0 for v in none.values())
    cosine = densityAnalysis.collinearity([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]], [[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]],
                                          [[-2, 0, 0], [0, 3, 0], [5, 0, 0], [2, 0, 0]])
    assert cosine[:3].tolist() == [-1.0, 0.0, 1.0] and np.isnan(cosine[3])


def test_symbol_is_declared_exported_and_bound():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pdbeda.h").read(), flags=re.S)
    assert re.search(r"\bint\s+pdbeda_bloblist_nearest\s*\(", text)
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "pdbeda_bloblist_nearest")
    assert "pdbeda_bloblist_nearest" in _native.EXPORTED_SYMBOLS and len(_native._SIGS["pdbeda_bloblist_nearest"][1]) == 8
    assert len(_native.EXPORTED_SYMBOLS) >= 64
    assert callable(_native.BlobList.nearest)


def test_dipole_mode_is_listed():
    from pdb_eda_amd import ccp4, densityAnalysis, singleStructure
    assert "dipole" in singleStructure.MODES and ("dipole", None) in singleStructure.TABLES
    header = singleStructure.TABLES[("dipole", None)][0](None)
    assert header == densityAnalysis.DensityAnalysis.blobDipoleHeader and len(header) == len(set(header)) == 18
    assert callable(ccp4.DeviceBlobs.nearestBlobs) and callable(densityAnalysis.DensityAnalysis.calculateBlobDipoles)
    with pytest.raises(ValueError):
        ccp4.DeviceBlobs([]).nearestBlobs(ccp4.DeviceBlobs([]), 1.5)          # (no segment: not a whole-map list)
