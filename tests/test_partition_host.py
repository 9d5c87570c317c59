"""The partition's yardstick and host glue without a GPU: tests/partition_checker.py against a hand-worked example, the residue
roll-up and the blob-ownership table on canned partition arrays."""
import types

import numpy as np

import partition_cases
import partition_checker


def _header(n=4):
    """A 4 x 4 x 4 box with unit spacing and the origin at 0: voxel (c, r, s) sits at (c, r, s)."""
    h = types.SimpleNamespace(ncrs=[n, n, n], uniqueNcrs=[n, n, n], crsInterval=[n, n, n])
    h.crs2xyzCoord = lambda crs: [float(crs[0]), float(crs[1]), float(crs[2])]
    return h


def test_checker_on_a_hand_worked_box():
    """Atoms 0 at (0, 0, 0) and 1 at (2, 0, 0), max distance 1, density = 1 + c + 4 r + 16 s (negated on the plane s = 1), cutoff 1.5.
    Along the row r = s = 0: voxel 0 is atom 0's (d = 0), voxel 1 is EQUIDISTANT (d = 1 to both: the lower index, atom 0, and the
    distance is exactly the maximum: inclusive), voxel 2 is atom 1's, voxel 3 is atom 1's at exactly d = 1.  Off the row, within
    d <= 1: (0,1,0) and (0,0,1) are atom 0's, (2,1,0) and (2,0,1) atom 1's.  Everything else is unowned."""
    h = _header()
    c, r, s = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    grid = np.zeros((4, 4, 4), dtype=np.float32)          # [s][r][c]
    grid[s, r, c] = 1 + c + 4 * r + 16 * s
    grid[1] *= -1
    got = partition_checker.partition(h, grid, [[0, 0, 0], [2, 0, 0]], 1.0, 1.5)
    owner = np.full((4, 4, 4), -1, dtype=np.int32)
    for (vc, vr, vs), who in {(0, 0, 0): 0, (1, 0, 0): 0, (0, 1, 0): 0, (0, 0, 1): 0, (2, 0, 0): 1, (3, 0, 0): 1, (2, 1, 0): 1, (2, 0, 1): 1}.items():
        owner[vs, vr, vc] = who
    assert np.array_equal(got["owner"], owner)
    # atom 0: densities 1, 2, 5, -17;  atom 1: 3, 4, 7, -19
    assert got["n"].tolist() == [4, 4] and got["sum"].tolist() == [-9.0, -5.0]
    assert got["n_pos"].tolist() == [2, 3] and got["sum_pos"].tolist() == [7.0, 14.0]          # (> 1.5: 2, 5 | 3, 4, 7)
    assert got["n_neg"].tolist() == [1, 1] and got["sum_neg"].tolist() == [-17.0, -19.0]
    assert int(got["tied"].sum()) == 1 and got["tied"].reshape(4, 4, 4)[0, 0, 1]
    assert int(got["on_sphere"].sum()) == 6          # every owned voxel but the two atoms' own
    rho = grid.astype(np.float64)
    free = owner < 0
    assert got["unowned_n"].tolist() == [56, int((rho[free] > 1.5).sum()), int((rho[free] < -1.5).sum())]
    assert got["unowned_n"].tolist() == [56, 42, 14]          # (48 - 6 voxels of the positive planes, 16 - 2 of the negative one)
    assert got["unowned_sum"].tolist() == [float(rho[free].sum()), float(rho[free][rho[free] > 1.5].sum()), float(rho[free][rho[free] < -1.5].sum()),
                                           float((rho[free] ** 2).sum())]
    # conservation, and NaN: owned and counted, in no sum and neither filter
    assert got["n"].sum() + got["unowned_n"][0] == 64 and got["sum"].sum() + got["unowned_sum"][0] == rho.sum()
    grid[0, 0, 0] = np.nan
    grid[3, 3, 3] = np.nan
    nan = partition_checker.partition(h, grid, [[0, 0, 0], [2, 0, 0]], 1.0, 0.0)
    assert nan["n"].tolist() == [4, 4] and nan["sum"][0] == -10.0 and nan["n_pos"][0] == 2 and nan["n_neg"][0] == 1
    assert nan["unowned_n"][0] == 56 and nan["unowned_sum"][0] == float(rho[free].sum()) - 64.0
    grid[0, 0, 1] = np.inf          # an infinite voxel, like a NaN one: owned (atom 0, where the density was 2) and counted, in no sum, in neither filter
    inf = partition_checker.partition(h, grid, [[0, 0, 0], [2, 0, 0]], 1.0, 0.0)
    assert inf["n"].tolist() == [4, 4] and inf["sum"][0] == -12.0 and inf["n_pos"][0] == 1 and inf["n_neg"][0] == 1
    grid[0, 0, 1] = 2.0
    # no atoms: everything is unowned
    none = partition_checker.partition(h, np.abs(grid), np.zeros((0, 3)), 1.0, 0.0)
    assert np.all(none["owner"] == -1) and none["unowned_n"].tolist() == [64, 62, 0] and len(none["n"]) == 0


def test_lattice_case_counts():
    from conftest import load_case
    z, header, grid = load_case("orth_rep")
    assert header.uniqueNcrs != header.ncrs
    assert len(partition_cases.lattice(header)) == 294
    assert partition_cases.random("orth_rep", header).shape == (32, 3)


def test_residue_rollup():
    from pdb_eda_amd import densityAnalysis
    n = np.array([3, 0, 5, 7, 1], dtype=np.int64)
    pos = np.array([0.5, 0.0, 1.25, 2.0, 0.125])
    off = np.array([0, 2, 2, 5], dtype=np.int64)          # residues of 2, 0 and 3 atoms
    got_n, got_pos = densityAnalysis._partitionRollup([n, pos], off)
    assert got_n.tolist() == [3, 0, 13] and got_n.dtype == np.int64
    assert got_pos.tolist() == [0.5, 0.0, 3.375]


def test_blob_owners():
    from pdb_eda_amd import densityAnalysis
    owner = np.full((2, 3, 4), -1, dtype=np.int32)          # [s][r][c]
    owner[0, 0, :] = [5, 5, 2, 2]
    owner[0, 1, :] = [2, -1, -1, 7]
    owner[1, 2, :] = [9, 9, 9, -1]
    row = lambda r, s: [[c, r, s] for c in range(4)]
    crs = np.array(row(0, 0) + row(1, 0) + row(2, 1) + row(2, 0), dtype=np.int32)
    off = np.array([0, 8, 8, 12, 16], dtype=np.int64)          # blob 0: two rows; blob 1: empty; blob 2: a row; blob 3: nobody's
    sizes, unowned, n_owners, main, main_voxels = densityAnalysis._blobOwners(owner, crs, off)
    assert sizes.tolist() == [8, 0, 4, 4] and unowned.tolist() == [2, 0, 1, 4] and n_owners.tolist() == [3, 0, 1, 0]
    assert main.tolist() == [2, -1, 9, -1] and main_voxels.tolist() == [3, 0, 3, 0]
    owner[0, 1, 1] = 5          # 5 and 2 now own three voxels each: the lower index
    assert densityAnalysis._blobOwners(owner, crs, off)[3].tolist() == [2, -1, 9, -1]
    owner[0, 0, 2] = 5
    assert densityAnalysis._blobOwners(owner, crs, off)[3].tolist() == [5, -1, 9, -1]


def test_methods_refuse_without_a_ratio_or_symmetry_atoms():
    """The analysis methods raise the usual RuntimeError without a densityElectronRatio and the blob table's ValueError when the
    symmetry list is empty (a file without operators) -- both before anything is asked of a device."""
    import pytest
    from conftest import load_analysis_case
    from pdb_eda_amd import densityAnalysis
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    an = densityAnalysis.DensityAnalysis("orth", None, None, st, pdb)
    calls = (lambda: an.calculateAtomPartitionDiscrepancies(), lambda: an.calculateResiduePartitionDiscrepancies(), lambda: an.partitionSummary(),
             lambda: an.calculateBlobOwnership([object()]))
    an._densityElectronRatio = 0.0          # aggregateCloud ran and found too few electrons
    for call in calls:
        with pytest.raises(RuntimeError, match="densityElectronRatio"):
            call()
    an._densityElectronRatio = 1.0
    an._symmetryAtomCoords = np.zeros((0, 3))
    an._symmetryAtoms = []
    for call in calls:
        with pytest.raises(ValueError, match="2-dimensional"):
            call()
