"""The nearest-atom partition on the MI355X path against tests/partition_checker.py, the plain numpy restatement of the contract
in include/pdbeda.h (pdbeda_map_partition).  Owners and counts are compared exactly (np.array_equal; the checker takes the voxel
coordinates from the device's crs2xyz, which tests/test_gpu_voxel.py pins bit for bit); a density sum within
1e-9 * n * max |rho| with n the voxels of that row -- the profile tests' bound: the project's 1e-9 for fp64 sums, scaled by what
the fixed-point quantum of the sums is derived from; the sum of squares within 1e-9 relative."""
import io
import json
import math

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import partition_cases
import partition_checker

pytestmark = pytest.mark.gpu

DISTANCES = (1.0, 2.0, 3.5)
_maps, _wanted = {}, {}


def device_map(name, gpu_ctx):
    from pdb_eda_amd import ccp4
    if name not in _maps:
        z, header, grid = load_case(name)
        _maps[name] = (header, grid, ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx))
    return _maps[name]


def checker(name, tag, dm, header, grid, xyz, max_distance, cutoff, chunk=4096):
    """The checker's answer, computed once per input and shared (never modified)."""
    key = (name, tag, max_distance, float(np.float32(cutoff)))
    if key not in _wanted:
        _wanted[key] = partition_checker.partition(header, grid, xyz, max_distance, cutoff, crs2xyz=dm._map.crs2xyz, chunk=chunk)
    return _wanted[key]


def assert_partition_equal(got, want, grid, what):
    """got: DeviceMap.partition(owners=True);  want: partition_checker.partition()."""
    assert np.array_equal(got["owner"], want["owner"]), what
    assert got["owner"].dtype == np.int32
    for mine, theirs in (("n", "n"), ("nPos", "n_pos"), ("nNeg", "n_neg"), ("unownedN", "unowned_n")):
        assert np.array_equal(got[mine], want[theirs]), (what, mine)
    top = float(np.abs(grid[np.isfinite(grid)]).max())
    for mine, theirs, count in (("sum", "sum", "n"), ("sumPos", "sum_pos", "n_pos"), ("sumNeg", "sum_neg", "n_neg")):
        err, bound = np.abs(got[mine] - want[theirs]), 1e-9 * want[count] * top
        if len(err):
            print("%s: max |%s - checker| = %.3g (bound at that atom %.3g)" % (what, mine, float(err.max()), float(bound[int(err.argmax())])))
        assert np.all(err <= bound), (what, mine)
        assert np.all(got[mine][want[count] == 0] == 0.0), (what, mine)          # an atom that owns nothing: exact zeros
    err, bound = np.abs(got["unownedSum"][:3] - want["unowned_sum"][:3]), 1e-9 * want["unowned_n"] * top
    print("%s: unowned |sum - checker| = %s (bounds %s)" % (what, err.tolist(), bound.tolist()))
    assert np.all(err <= bound), what
    sq, sq_want = float(got["unownedSum"][3]), float(want["unowned_sum"][3])
    print("%s: unowned sum_sq %.17g, checker %.17g" % (what, sq, sq_want))
    assert abs(sq - sq_want) <= 1e-9 * abs(sq_want), what


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_golden_maps_against_checker(gpu_ctx, name):
    header, grid, dm = device_map(name, gpu_ctx)
    xyz = partition_cases.random(name, header)
    box = int(np.prod(header.uniqueNcrs))
    for max_distance in DISTANCES:
        for cut in (0.0, dm.meanDensity + 1.5 * dm.stdDensity):
            want = checker(name, "random", dm, header, grid, xyz, max_distance, cut)
            owned = int(want["n"].sum())
            print("%s d=%g cut=%.3g: checker owned / unowned = %d / %d, %d atoms own something" % (name, max_distance, cut, owned, box - owned,
                                                                                                  int((want["n"] > 0).sum())))
            assert 0 < owned < box and owned + int(want["unowned_n"][0]) == box          # (a vacuous comparison cannot pass)
            if max_distance == 3.5:
                assert int((want["n"] > 0).sum()) >= 27
            if cut > 0:
                assert 0 < want["n_pos"].sum() < owned and 0 < want["unowned_n"][1] < want["unowned_n"][0]
            got = dm._map.partition(xyz, max_distance, cut, owners=True)
            assert_partition_equal(got, want, grid, "%s d=%g cut=%.3g" % (name, max_distance, cut))
            again = dm.partition([list(p) for p in xyz], max_distance, cut, owners=True)          # the object model hands the same arrays on
            assert all(np.array_equal(again[k], got[k]) for k in got)
            assert "owner" not in dm.partition(xyz, max_distance, cut)


@pytest.mark.parametrize("max_distance,min_tied,min_on_sphere,min_unowned", [(1.0, 749, 966, 1), (2.0, 10559, 0, 120)])
def test_ties_and_the_sphere_boundary(gpu_ctx, max_distance, min_tied, min_on_sphere, min_unowned):
    """orth_rep has spacing 0.5 (exact in binary) and the lattice atoms sit on voxel centres 2.0 apart: voxels half way between two of
    them are equidistant to the bit (the lowest index owns), and whole shells of voxels lie exactly on the sphere (inclusive)."""
    header, grid, dm = device_map("orth_rep", gpu_ctx)
    xyz = partition_cases.lattice(header)
    assert len(xyz) == 294
    want = checker("orth_rep", "lattice", dm, header, grid, xyz, max_distance, 0.0)
    print("d=%g: %d tied voxels, %d exactly on the sphere, %d unowned" % (max_distance, int(want["tied"].sum()), int(want["on_sphere"].sum()), int(want["unowned_n"][0])))
    assert want["tied"].sum() >= min_tied and want["on_sphere"].sum() >= min_on_sphere and want["unowned_n"][0] >= min_unowned
    got = dm._map.partition(xyz, max_distance, 0.0, owners=True)
    assert_partition_equal(got, want, grid, "orth_rep lattice d=%g" % max_distance)
    # another order of the atoms moves only the tied voxels, and no bit of the rows of atoms that own none of them
    both = np.concatenate([xyz, partition_cases.random("orth_rep", header)])
    base = dm._map.partition(both, max_distance, 0.0, owners=True)
    tied = checker("orth_rep", "lattice+random", dm, header, grid, both, max_distance, 0.0)["tied"].reshape(base["owner"].shape)
    perm = np.random.default_rng(7).permutation(len(both))
    moved = dm._map.partition(both[perm], max_distance, 0.0, owners=True)
    back = np.where(moved["owner"] >= 0, perm[np.maximum(moved["owner"], 0)], -1)
    assert np.array_equal(back[~tied], base["owner"][~tied]) and np.any(back[tied] != base["owner"][tied])
    touched = np.union1d(base["owner"][tied], back[tied])
    rest = np.setdiff1d(np.arange(len(both)), touched)
    print("d=%g: %d of %d atoms own no tied voxel in either order" % (max_distance, len(rest), len(both)))
    assert len(rest) >= 1 and base["n"][rest].sum() > 0
    inverse = np.argsort(perm)
    for k in ("n", "sum", "nPos", "sumPos", "nNeg", "sumNeg"):
        assert moved[k][inverse][rest].tobytes() == base[k][rest].tobytes(), k
    assert moved["unownedN"].tobytes() == base["unownedN"].tobytes() and moved["unownedSum"].tobytes() == base["unownedSum"].tobytes()


def test_crowded_cell(gpu_ctx):
    """More atoms around one spot than the kernel stages at a time (512), so the tiles near it run the staging buffer several times and
    send their sums to global memory themselves: 3 000 atoms on one coordinate (the lowest index owns, the others are exact zeros) and,
    among them in the list, 600 distinct atoms 0.4 A apart around the same spot (about the voxel spacing, so most own a voxel), so that the best (d2, index) carried from run to run
    and the sums belong to many different owners inside one overflowing tile."""
    header, grid, dm = device_map("orth", gpu_ctx)
    spot = np.array(header.crs2xyzCoord([int(header.ncrs[k]) // 2 for k in range(3)]), dtype=np.float64) + 0.1
    k = np.arange(600)
    cloud = spot + 0.4 * np.stack([k % 10 - 4.5, (k // 10) % 10 - 4.5, k // 100 - 2.5], axis=1)
    xyz = np.concatenate([np.tile(spot, (1500, 1)), cloud[:300], np.tile(spot, (1500, 1)), cloud[300:], partition_cases.random("orth", header)])
    same = np.concatenate([np.arange(1, 1500), np.arange(1800, 3300)])          # the copies of atom 0
    want = checker("orth", "crowded", dm, header, grid, xyz, 3.5, 0.0, chunk=512)
    owners_near = int((want["n"][np.concatenate([np.arange(1500, 1800), np.arange(3300, 3600)])] > 0).sum())
    print("crowded: atom 0 owns %d voxels, %d of the 600 close atoms own something" % (int(want["n"][0]), owners_near))
    assert np.all(want["n"][same] == 0) and owners_near >= 100
    got = dm._map.partition(xyz, 3.5, 0.0, owners=True)
    assert_partition_equal(got, want, grid, "orth crowded")
    for name in ("n", "sum", "nPos", "sumPos", "nNeg", "sumNeg"):
        assert not got[name][same].any(), name


def test_exactly_one_buffer_of_atoms(gpu_ctx):
    """512 distinct atoms -- exactly one staging buffer -- inside one cube of 1.2 A and none elsewhere: every tile near them fills the
    buffer to the brim and finds nothing behind it."""
    header, grid, dm = device_map("tric", gpu_ctx)
    spot = np.array(header.crs2xyzCoord([int(header.ncrs[k]) // 2 for k in range(3)]), dtype=np.float64)
    k = np.arange(512)
    xyz = spot + 0.15 * np.stack([k % 8 - 3.5, (k // 8) % 8 - 3.5, k // 64 - 3.5], axis=1)
    want = checker("tric", "brim", dm, header, grid, xyz, 2.0, 0.0, chunk=512)
    print("brim: %d atoms own something, %d voxels owned" % (int((want["n"] > 0).sum()), int(want["n"].sum())))
    assert (want["n"] > 0).sum() >= 100 and 0 < want["unowned_n"][0]
    assert_partition_equal(dm._map.partition(xyz, 2.0, 0.0, owners=True), want, grid, "tric brim")


@pytest.mark.parametrize("name", ["orth_rep", "wide", "tric"])
def test_conservation(gpu_ctx, name):
    header, grid, dm = device_map(name, gpu_ctx)
    xyz = partition_cases.random(name, header)
    box = partition_checker.box_grid(header, grid).astype(np.float64)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    got = dm._map.partition(xyz, 2.0, cut)
    assert got["n"].sum() + got["unownedN"][0] == box.size
    assert got["nPos"].sum() + got["unownedN"][1] == np.count_nonzero(box > float(np.float32(cut)))
    assert got["nNeg"].sum() + got["unownedN"][2] == np.count_nonzero(box < -float(np.float32(cut)))
    total, exact = math.fsum(got["sum"].tolist()) + float(got["unownedSum"][0]), math.fsum(box.reshape(-1).tolist())
    print("%s: |sum of the parts - fsum(box)| = %.3g (bound %.3g)" % (name, abs(total - exact), 1e-9 * box.size * float(np.abs(box).max())))
    assert abs(total - exact) <= 1e-9 * box.size * float(np.abs(box).max())


def test_agrees_with_region_sums(gpu_ctx):
    """One isolated atom on the middle voxel of orth_rep, radius 2.0: R and C of the sphere box are exact there, the box covers the
    sphere and the sphere lies inside the non-repeating box -- the atom's partition row IS its region."""
    header, grid, dm = device_map("orth_rep", gpu_ctx)
    xyz = np.array([header.crs2xyzCoord([int(header.uniqueNcrs[k]) // 2 for k in range(3)])], dtype=np.float64)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    pos, neg, cnt, valid = dm._map.region_sums(xyz, np.full(1, 2.0, dtype=np.float32), np.array([0, 1], dtype=np.int64), cut)
    got = dm._map.partition(xyz, 2.0, cut)
    top = float(np.abs(grid).max())
    print("n %d / %d, pos %.17g / %.17g, neg %.17g / %.17g" % (got["n"][0], cnt[0], got["sumPos"][0], pos[0], got["sumNeg"][0], neg[0]))
    assert valid[0] and cnt[0] > 100 and got["n"][0] == cnt[0]
    assert abs(got["sumPos"][0] - pos[0]) <= 1e-9 * got["nPos"][0] * top and abs(got["sumNeg"][0] - neg[0]) <= 1e-9 * got["nNeg"][0] * top
    assert got["nPos"][0] > 0 and got["nNeg"][0] > 0


def test_bit_identical_from_run_to_run_and_with_far_atoms(gpu_ctx):
    header, grid, dm = device_map("orth", gpu_ctx)
    xyz = partition_cases.random("orth", header)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    first, second = dm._map.partition(xyz, 3.5, cut, owners=True), dm._map.partition(xyz, 3.5, cut, owners=True)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    corners = np.array([header.crs2xyzCoord([c, r, s]) for c in (0, header.ncrs[0] - 1) for r in (0, header.ncrs[1] - 1) for s in (0, header.ncrs[2] - 1)])
    far = np.concatenate([corners.max(axis=0) + [[50.0, 0, 0], [0, 60.0, 0], [5.0, 5.0, 5.0]], corners.min(axis=0) - [[4.0, 4.0, 4.0], [1e6, 0, 0]]])
    more = dm._map.partition(np.concatenate([xyz, far]), 3.5, cut, owners=True)
    for k in ("n", "sum", "nPos", "sumPos", "nNeg", "sumNeg"):
        assert more[k][:len(xyz)].tobytes() == first[k].tobytes() and not more[k][len(xyz):].any(), k
    for k in ("owner", "unownedN", "unownedSum"):
        assert more[k].tobytes() == first[k].tobytes(), k


def test_arguments(gpu_ctx):
    from pdb_eda_amd import _native
    header, grid, dm = device_map("orth", gpu_ctx)
    xyz = partition_cases.random("orth", header)
    want = dm._map.partition(xyz, 2.0, 0.0, owners=True)
    bad_xyz = xyz.copy()
    bad_xyz[5, 1] = np.inf
    for args in ((xyz, 0.0, 0.0), (xyz, -1.0, 0.0), (xyz, np.inf, 0.0), (xyz, np.nan, 0.0), (xyz, 2.0, np.nan), (xyz, 2.0, -0.5), (bad_xyz, 2.0, 0.0)):
        with pytest.raises(_native.PdbedaError):
            dm._map.partition(*args)
        again = dm._map.partition(xyz, 2.0, 0.0, owners=True)          # the context is not poisoned
        assert all(np.array_equal(again[k], want[k]) for k in want)
    # 2^31 atoms: refused before the coordinates are read (a raw call: no array of that length exists)
    import ctypes
    none = ctypes.c_void_p(None)
    for count in (2 ** 31, 2 ** 40):
        rc = dm._map._ctx._lib.pdbeda_map_partition(dm._map._h, xyz.ctypes.data_as(ctypes.c_void_p), count, ctypes.c_float(2.0), ctypes.c_float(0.0),
                                                    none, none, none, none, none, none, none, none, none)
        with pytest.raises(_native.PdbedaError):
            dm._map._ctx.check(rc, "pdbeda_map_partition")
        again = dm._map.partition(xyz, 2.0, 0.0, owners=True)
        assert all(np.array_equal(again[k], want[k]) for k in want)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    empty = dm._map.partition(np.zeros((0, 3)), 2.0, cut, owners=True)
    box = partition_checker.box_grid(header, grid).astype(np.float64)
    assert np.all(empty["owner"] == -1) and empty["owner"].shape == box.shape and all(empty[k].shape == (0,) for k in ("n", "sum", "nPos", "sumPos", "nNeg", "sumNeg"))
    c32 = float(np.float32(cut))
    assert empty["unownedN"].tolist() == [box.size, int((box > c32).sum()), int((box < -c32).sum())]
    top = float(np.abs(box).max())
    for k, exact in enumerate((box, box[box > c32], box[box < -c32])):
        assert abs(empty["unownedSum"][k] - math.fsum(exact.reshape(-1).tolist())) <= 1e-9 * exact.size * top
    assert abs(empty["unownedSum"][3] - math.fsum((box ** 2).reshape(-1).tolist())) <= 1e-9 * math.fsum((box ** 2).reshape(-1).tolist())


def test_nan_and_infinite_voxels(gpu_ctx):
    """A NaN or infinite voxel is owned and counted in n; it enters no density sum and neither filter (the map's own quantum is
    refused then: the partition derives one from the finite voxels of the box)."""
    from pdb_eda_amd import ccp4, synthetic
    spec = synthetic.MapSpec(ncrs=(37, 22, 19), spacing=0.7)
    grid = synthetic.noise_grid(spec, seed=11, sigma_voxels=1.5).astype(np.float32)
    xyz_crs = [[18, 11, 9], [3, 4, 5]]
    grid[9, 11, 18] = np.nan          # on an atom
    grid[0, 0, 0] = np.nan            # far from both
    grid[9, 11, 19] = np.inf          # beside the first atom
    grid[5, 4, 4] = -np.inf           # beside the second
    grid[18, 21, 36] = np.inf         # far from both
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "nan", ctx=gpu_ctx)
    xyz = np.array([dm.header.crs2xyzCoord(v) for v in xyz_crs], dtype=np.float64)
    want = partition_checker.partition(dm.header, grid, xyz, 2.0, 0.25, crs2xyz=dm._map.crs2xyz)
    assert want["owner"][9, 11, 18] == 0 and want["owner"][9, 11, 19] == 0 and want["owner"][5, 4, 4] == 1
    assert want["owner"][0, 0, 0] == -1 and want["owner"][18, 21, 36] == -1
    assert np.isfinite(want["sum"]).all() and np.isfinite(want["unowned_sum"]).all()
    rest = grid.copy()
    rest[~np.isfinite(rest)] = 0.0          # the same map with those voxels at 0, cutoff 0.25: the same counts of the filters
    plain = partition_checker.partition(dm.header, rest, xyz, 2.0, 0.25, crs2xyz=dm._map.crs2xyz)
    assert np.array_equal(plain["n_pos"], want["n_pos"]) and np.array_equal(plain["n_neg"], want["n_neg"]) and np.array_equal(plain["n"], want["n"])
    assert_partition_equal(dm._map.partition(xyz, 2.0, 0.25, owners=True), want, grid, "nan and infinite voxels")


# ---- the analysis surface ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analysis(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    an = densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb)
    grid = np.asarray(z["diff"], dtype=np.float32)
    want = partition_checker.partition(diff.header, grid, np.asarray(an.symmetryAtomCoords, dtype=np.float64), 3.5, diff.meanDensity + 3.0 * diff.stdDensity,
                                       crs2xyz=diff._map.crs2xyz, chunk=1024)
    return an, grid, want


def test_analysis_tables(analysis):
    from pdb_eda_amd import singleStructure
    an, grid, want = analysis
    ratio = an.densityElectronRatio
    assert ratio
    top = float(np.abs(grid).max())
    atoms = list(an.biopdbObj.get_atoms())
    sym = an.symmetryAtoms
    own = np.nonzero(sym._ident)[0]
    row_of = {int(sym._idx[j]): int(j) for j in own}          # structure atom -> its place in the symmetry list
    header = an.atomPartitionHeader
    table = an.calculateAtomPartitionDiscrepancies()
    assert len(table) == len(atoms) and all(len(row) == len(header) for row in table) and len(row_of) > 0.5 * len(atoms)
    assert header[:6] == an.atomRegionDiscrepancyHeader[:6] and [row[:6] for row in table] == [row[:6] for row in an.calculateAtomRegionDiscrepancies(3.5)]
    for k, row in enumerate(table):
        r = dict(zip(header, row))
        j = row_of.get(k)
        n, pos, neg, n_pos, n_neg = (int(want["n"][j]), want["sum_pos"][j], want["sum_neg"][j], int(want["n_pos"][j]), int(want["n_neg"][j])) if j is not None else (0, 0.0, 0.0, 0, 0)
        assert r["num_voxels"] == n
        assert abs(r["positive_discrepancy"] - pos) <= 1e-9 * n_pos * top and abs(r["negative_discrepancy"] - neg) <= 1e-9 * n_neg * top
        assert r["abs_discrepancy"] == r["positive_discrepancy"] - r["negative_discrepancy"] and r["net_discrepancy"] == r["positive_discrepancy"] + r["negative_discrepancy"]
        for name in ("positive", "negative", "abs", "net"):
            assert r["num_electrons_%s_discrepancy" % name] == r["%s_discrepancy" % name] / ratio
    assert sum(row[6] for row in table) > 0 and any(row[7] > 0 for row in table) and any(row[9] < 0 for row in table)
    # residues: the sum of their atoms' rows
    by_residue = an.calculateResiduePartitionDiscrepancies()
    residues = list(an.biopdbObj.get_residues())
    assert len(by_residue) == len(residues) and [row[:5] for row in by_residue] == [row[:5] for row in an.calculateResidueRegionDiscrepancies(3.5)]
    at = 0
    for row, residue in zip(by_residue, residues):
        mine = table[at:at + len(residue)]
        at += len(residue)
        assert row[5] == sum(m[6] for m in mine)
        for col, src in ((6, 7), (8, 9)):
            assert abs(row[col] - math.fsum(m[src] for m in mine)) <= 1e-12 * max(1.0, abs(row[col]))
    assert at == len(atoms)
    # the three classes add up to the box; the unowned mean and deviation against numpy on the checker's unowned voxels
    summary = an.partitionSummary()
    box = partition_checker.box_grid(an.diffDensityObj.header, grid).astype(np.float64)
    assert summary["box_voxels"] == box.size == summary["asymmetric_unit_voxels"] + summary["symmetry_voxels"] + summary["unowned_voxels"]
    assert summary["asymmetric_unit_voxels"] == int(want["n"][own].sum()) and summary["unowned_voxels"] == int(want["unowned_n"][0]) > 0
    free = box[want["owner"] < 0]
    print("unowned mean %.17g (numpy %.17g), std %.17g (numpy %.17g); map %.6g / %.6g" % (summary["unowned_mean"], free.mean(), summary["unowned_std"], free.std(),
                                                                                       summary["map_mean"], summary["map_std"]))
    assert abs(summary["unowned_mean"] - free.mean()) <= 1e-9 * np.abs(free).max() and abs(summary["unowned_std"] - free.std()) <= 1e-9 * free.std()
    assert summary["unowned_fraction"] == summary["unowned_voxels"] / box.size and summary["map_mean"] == an.diffDensityObj.meanDensity
    # who owns the green blobs: recomputed from the checker's owner volume
    green = an.diffDensityObj.createFullBlobList(an.diffDensityObj.meanDensity + 3.0 * an.diffDensityObj.stdDensity)
    stats = an.calculateAtomSpecificBlobStatistics(an.diffDensityObj.createFullBlobList(an.diffDensityObj.meanDensity + 3.0 * an.diffDensityObj.stdDensity))
    owned_by = an.calculateBlobOwnership(green)
    assert len(owned_by) == len(green) == len(stats) > 0 and [row[0] for row in owned_by] == [row[3] for row in stats]
    names = an.blobOwnershipHeader
    for row, blob in zip(owned_by, green):
        r = dict(zip(names, row))
        who = np.array([want["owner"][s, rr, c] for c, rr, s in blob.crsList])
        ids, counts = np.unique(who[who >= 0], return_counts=True)
        assert r["num_voxels"] == len(who) and r["unowned_voxels"] == int((who < 0).sum()) and r["num_owner_atoms"] == len(ids)
        if len(ids):
            main = int(ids[np.argmax(counts)])          # (the first maximum: the lowest symmetry-atom index)
            atom = atoms[int(sym._idx[main])]
            assert r["main_owner_voxels"] == int(counts.max()) and r["atom_name"] == atom.name and r["residue_name"] == atom.parent.resname
            assert r["residue_number"] == atom.parent.id[1] and r["chain"] == atom.parent.parent.id and tuple(r["atom_symmetry"]) == tuple(int(v) for v in sym._sym[main])
        else:
            assert r["main_owner_voxels"] == 0 and r["atom_name"] is None and r["atom_symmetry"] is None
    # `single` mode: the four levels, through JSON and CSV
    for level, reference in (("atom", table), ("residue", by_residue), ("summary", None), ("blob", None)):
        head, rows = singleStructure.rows(an, "partition", level, green=True)
        if reference is not None:
            assert rows == reference
        elif level == "summary":
            assert len(rows) == 1 and dict(zip(head, rows[0])) == summary
        else:
            assert head == names and [row[:7] + row[8:] for row in rows] == [row[:7] + row[8:] for row in owned_by]
        assert len(rows) > 0 and all(len(row) == len(head) for row in rows)
        assert json.loads(singleStructure.dumps(head, rows, "json")) == [dict(zip(head, row)) for row in rows]
        text = singleStructure.dumps(head, rows, "csv").splitlines()
        assert text[0] == ",".join(head) and text[1:] == [",".join(map(str, row)) for row in rows]
    with pytest.raises(ValueError):
        singleStructure.rows(an, "partition", "domain")
