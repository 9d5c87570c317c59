"""pdbeda_bloblist_moments and the shape columns built on it, on the MI355X path against tests/blobshape_checker.py, the plain numpy
restatement of the contract in include/pdbeda.h.  The voxel lists come from the product's own voxels() (tests/test_gpu_voxel.py pins those
bit for bit) and the grid from the fixture.  Box, extreme voxel and the integer sums are compared exactly; a weighted sum within
1e-9 * n * max |rho| * D^2 (n the blob's voxels, D its largest box width in voxels; sw itself within 1e-9 * n * max |rho|): the project's
bound for fixed-point sums, as in the partition and profile tests, times the largest multiplier a product of two offsets can have; an
Angstrom quantity within 1e-9 * (box diagonal in A)^2."""
import csv
import io
import json

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import blobshape_checker as checker

pytestmark = pytest.mark.gpu

CHUNK = 2048                                   # list positions of one workgroup: BS_CHUNK of pdb_eda_amd/csrc/pdbeda_blobshape.h
MOMENT_COLUMNS = ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2", "sw", "sw1", "sw2")
_maps, _big = {}, {}


def device_map(name, gpu_ctx):
    from pdb_eda_amd import ccp4
    if name not in _maps:
        z, header, grid = load_case(name)
        _maps[name] = (header, grid, ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx))
    return _maps[name]


def synthetic_map(spec, grid, name, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=gpu_ctx)


def big_map(gpu_ctx):
    """96^3 smooth noise, cut at mean + 1 sigma: one blob of more than ten chunks among hundreds of crumbs (the counts are asserted in the test)."""
    from pdb_eda_amd import synthetic
    if not _big:
        spec = synthetic.MapSpec(ncrs=(96, 96, 96), spacing=0.4)
        grid = synthetic.noise_grid(spec, seed=11, sigma_voxels=1.5)
        dm = synthetic_map(spec, grid, "big", gpu_ctx)
        _big.update(grid=grid, dm=dm, cut=dm.meanDensity + 1.0 * dm.stdDensity)
    return _big["dm"].header, _big["grid"], _big["dm"], _big["cut"]


def assert_bytes_equal(a, b, what):
    for k in MOMENT_COLUMNS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def assert_matches_checker(header, grid, bl, whole_map, what):
    """bl: a _native.BlobList.  Returns (moments, checker's columns)."""
    from pdb_eda_amd import ccp4
    crs, off = bl.voxels()
    want = checker.shape(header, grid, crs, off, whole_map)
    got = bl.moments()
    nb = len(want["n"])
    assert len(bl) == nb and np.array_equal(bl.stats()["n"], want["n"]), what
    assert got["boxLo"].dtype == got["boxHi"].dtype == got["extremeCrs"].dtype == np.int32 and got["extreme"].dtype == np.float32
    assert got["s1"].dtype == got["s2"].dtype == np.int64 and got["s1"].shape == (nb, 3) and got["s2"].shape == (nb, 6)
    for k in ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2"):
        assert np.array_equal(got[k], want[k]), (what, k)
    if nb == 0:
        return got, want
    top = float(np.abs(grid).max())
    n = want["n"].astype(np.float64)
    width = (want["boxHi"].astype(np.int64) - want["boxLo"] + 1).max(axis=1).astype(np.float64)
    err = np.abs(got["sw"] - want["sw"])
    print("%s: %d blobs, largest %d voxels; max |sw - checker| = %.3g (bound there %.3g)" % (what, nb, int(n.max()), float(err.max()),
                                                                                             1e-9 * n[int(err.argmax())] * top))
    assert np.all(err <= 1e-9 * n * top), (what, "sw")
    for k in ("sw1", "sw2"):
        err, bound = np.abs(got[k] - want[k]).max(axis=1), 1e-9 * n * top * width ** 2
        print("%s: max |%s - checker| = %.3g (bound there %.3g)" % (what, k, float(err.max()), float(bound[int(err.argmax())])))
        assert np.all(err <= bound), (what, k)
    single = want["n"] == 1
    assert not got["s1"][single].any() and not got["s2"][single].any() and not got["sw1"][single].any() and not got["sw2"][single].any(), what
    # the Angstrom columns of the finishing step against the checker's sums over the voxels' xyz
    cols = ccp4.blobShapeFinish(header, want["n"], got, whole_map)
    tol = 1e-9 * want["boxDiagonal"] ** 2
    dense = want["sw"] > 0                                                   # (no density, no weighted moments: NaN on both sides)
    for k, power in (("secondMomentXyz", 1), ("weightedSecondMomentXyz", 1), ("principalLengths", 2), ("weightedPrincipalLengths", 2), ("weightedCentroid", 1),
                     ("extremeXyz", 1), ("boxExtent", 1)):
        keep = dense if k.startswith("weighted") else np.ones(nb, bool)
        err = np.abs(cols[k] ** power - want[k] ** power).reshape(nb, -1).max(axis=1)
        assert np.isnan(cols[k][~keep]).all() and np.isnan(want[k][~keep]).all(), (what, k)
        if keep.any():
            worst = int(np.where(keep, err / tol, -1.0).argmax())
            print("%s: max |%s - checker| / bound = %.3g (blob of %d voxels)" % (what, k, float(err[worst] / tol[worst]), int(n[worst])))
        assert np.all(err[keep] <= tol[keep]), (what, k)
    assert np.array_equal(cols["onBorder"], want["onBorder"]), what
    err, bound = np.abs(cols["anisotropy"] - want["anisotropy"]), checker.anisotropy_bound(want, tol)          # (what the bound on the variances allows, per blob)
    print("%s: max |anisotropy - checker| / bound = %.3g" % (what, float((err / bound).max())))
    assert np.all(err <= bound), (what, "anisotropy")
    return got, want


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_golden_maps_against_checker(gpu_ctx, name):
    header, grid, dm = device_map(name, gpu_ctx)
    blobs, largest, border = 0, 0, 0
    for k in (1.5, 3.0):
        cut = dm.meanDensity + k * dm.stdDensity
        green, red = dm._map.full_blobs_pm(cut, -cut)
        for tag, bl in (("green", green), ("red", red), ("green alone", dm._map.full_blobs(cut)), ("red alone", dm._map.full_blobs(-cut))):
            got, want = assert_matches_checker(header, grid, bl, True, "%s %g sigma %s" % (name, k, tag))
            if "alone" not in tag:
                blobs += len(want["n"])
                largest = max(largest, int(want["n"].max(initial=0)))
                border += int(want["onBorder"].sum())
    print("%s: %d blobs in the fused lists, the largest of %d voxels, %d on the border" % (name, blobs, largest, border))
    assert largest > 64 and blobs >= 20 and border >= 1                      # (a vacuous comparison cannot pass)


def test_blob_split_over_many_workgroups(gpu_ctx):
    header, grid, dm, cut = big_map(gpu_ctx)
    bl = dm._map.full_blobs(cut)
    got, want = assert_matches_checker(header, grid, bl, True, "96^3 at 1 sigma")
    n = want["n"]
    print("96^3: %d blobs, the largest of %d voxels = %.1f chunks, %d single voxels" % (len(n), int(n.max()), n.max() / CHUNK, int((n == 1).sum())))
    assert len(n) >= 100 and n.max() > 10 * CHUNK and (n == 1).sum() >= 30
    assert (np.diff(bl.voxels()[1]) > 0).all()


def test_run_to_run_identity(gpu_ctx):
    """The same map labelled twice into fresh lists: every column to the byte (the voxel lists themselves may differ in order)."""
    header, grid, dm, cut = big_map(gpu_ctx)
    first = dm._map.full_blobs(cut).moments()
    assert len(first["sw"]) >= 100
    assert_bytes_equal(dm._map.full_blobs(cut).moments(), first, "96^3 again")
    green, red = dm._map.full_blobs_pm(cut, -cut)
    assert_bytes_equal(green.moments(), first, "96^3 fused green")
    again = dm._map.full_blobs_pm(cut, -cut)
    assert_bytes_equal(again[1].moments(), red.moments(), "96^3 fused red")


@pytest.mark.parametrize("name", ["orth", "orth_sub", "hex"])
def test_fused_red_list_is_the_single_red_call(gpu_ctx, name):
    header, grid, dm = device_map(name, gpu_ctx)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    green, red = dm._map.full_blobs_pm(cut, -cut)
    red_first = red.moments()                                                # (asked before the green list: the red rows start at the job's rank_lo)
    assert len(red_first["sw"]) >= 5 and len(green) >= 5
    assert_bytes_equal(red_first, dm._map.full_blobs(-cut).moments(), name + " red")
    assert_bytes_equal(green.moments(), dm._map.full_blobs(cut).moments(), name + " green")
    green.free()                                                             # the red list outlives the list that owns the job's arena
    fresh = dm._map.full_blobs_pm(cut, -cut)[1]
    assert_bytes_equal(red.moments(), red_first, name + " red, kept")
    assert_bytes_equal(fresh.moments(), red_first, name + " red, fresh")
    late_green, late_red = dm._map.full_blobs_pm(cut, -cut)
    late_green.free()                                                        # ... also when its rows are made only then
    assert_bytes_equal(late_red.moments(), red_first, name + " red, after the green list has gone")


@pytest.mark.parametrize("name", ["orth_sub", "hex", "orth_rep"])
def test_sphere_and_list_batches(gpu_ctx, name):
    """Spheres around the corner voxel of the cell -- raw crs go negative and wrap (orth_sub: onto voxels that are not stored) -- and explicit
    voxel sets with duplicates, one of them a whole cell away."""
    header, grid, dm = device_map(name, gpu_ctx)
    corner = [header.crs2xyzCoord(c) for c in ([0, 0, 0], [1, 0, 1], [0, 2, 0], [3, 3, 3], [header.ncrs[0] - 1, 0, 0], [-2, -1, 0])]
    xyz = np.array(corner, dtype=np.float32).astype(np.float64)
    offsets = np.array([0, 1, 3, 4, 6], dtype=np.int64)
    total, negative = 0, False
    for cut in (0.0, dm.meanDensity + 1.5 * dm.stdDensity):
        bl = dm._map.sphere_blobs(xyz, np.full(len(xyz), 2.0, np.float32), offsets, cut)
        got, want = assert_matches_checker(header, grid, bl, False, "%s spheres cut %.3g" % (name, cut))
        total += len(want["n"])
        negative = negative or bool((want["boxLo"] < 0).any())
    assert total >= 6 and negative
    crs, off = bl.voxels()                                                   # the blobs of the last batch as explicit sets
    assert len(crs) >= 20
    shift = np.array([-int(header.crsInterval[0]), 0, int(header.crsInterval[2])])
    sets = [np.concatenate([crs, crs[: len(crs) // 2]]), np.concatenate([crs[::-1] + shift, crs[:3] + shift, crs[:3] + shift])]
    lb = dm._map.list_blobs(np.concatenate(sets), np.array([0, len(sets[0]), len(sets[0]) + len(sets[1])], dtype=np.int64))
    got, want = assert_matches_checker(header, grid, lb, False, name + " lists with duplicates")
    half = len(want["n"]) // 2                                               # the second group is the first one, moved (spheres that touch have merged)
    assert half >= 1 and len(want["n"]) == 2 * half and int(want["n"].sum()) == 2 * len(np.unique(crs, axis=0))          # duplicates collapse
    assert np.array_equal(got["boxLo"][half:], got["boxLo"][:half] + shift) and got["s1"][half:].tobytes() == got["s1"][:half].tobytes()
    assert got["s2"][half:].tobytes() == got["s2"][:half].tobytes()


def test_plateau_ties(gpu_ctx):
    """Values exact in float32.  A slab of 40 x 40 x 8 voxels at 2.0 (more than six chunks: its ties meet across waves and workgroups) with five
    voxels at 3.0 inside it; a small plateau at 2.0 where every voxel ties; a plateau at -2.0 for the red list."""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(48, 44, 14), spacing=0.5)
    grid = np.zeros((14, 44, 48), dtype=np.float32)
    grid[2:10, 2:42, 3:43] = 2.0
    peaks = [(30, 7, 5), (9, 40, 2), (9, 12, 9), (41, 3, 3), (9, 12, 4)]     # (c, r, s); the first in (c, r, s) order is (9, 12, 4)
    for c, r, s in peaks:
        grid[s, r, c] = 3.0
    grid[12:14, 0:3, 44:47] = 2.0                                            # all equal: the first voxel is (44, 0, 12)
    grid[12:14, 30:40, 5:20] = -2.0                                          # red: the first voxel is (5, 30, 12)
    dm = synthetic_map(spec, grid, "plateau", gpu_ctx)
    seen = []
    for run in range(5):
        green, red = dm._map.full_blobs_pm(0.5, -0.5)
        got, want = assert_matches_checker(dm.header, grid, green, True, "plateau green, list %d" % run)
        got_red, _ = assert_matches_checker(dm.header, grid, red, True, "plateau red, list %d" % run)
        assert want["n"].tolist() == [12800, 18] and got["extremeCrs"].tolist() == [[9, 12, 4], [44, 0, 12]] and got["extreme"].tolist() == [3.0, 2.0]
        assert got_red["extremeCrs"].tolist() == [[5, 30, 12]] and got_red["extreme"].tolist() == [-2.0]
        seen.append((got, got_red))
    for got, got_red in seen[1:]:
        assert_bytes_equal(got, seen[0][0], "plateau green")
        assert_bytes_equal(got_red, seen[0][1], "plateau red")


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_weighted_centroid_is_the_reference_centroid(gpu_ctx, name):
    """Every blob of a whole-map list has one sign, so box_lo + sw1 / sw through crs2xyz's linear map is the centroid column of
    pdbeda_bloblist_stats -- the column the reference pins."""
    header, grid, dm = device_map(name, gpu_ctx)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    count = 0
    for blobs in dm.createFullBlobLists(cut):
        shape, listed = blobs.shapeColumns(), blobs.columns()
        step = header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3)))
        diagonal = np.linalg.norm((shape["boxHi"].astype(np.float64) - shape["boxLo"] + 1).dot(step), axis=1)
        err = np.abs(shape["weightedCentroid"] - listed["centroid"]).max(axis=1)
        print("%s: max |weighted centroid - centroid| / (1e-9 diagonal) = %.3g over %d blobs" % (name, float((err / (1e-9 * diagonal)).max()), len(err)))
        assert np.all(err <= 1e-9 * diagonal)
        count += len(err)
        # the objects read the same columns, lazily and read-only
        blob = blobs[len(blobs) // 2]
        assert blob.principalLengths == shape["principalLengths"][len(blobs) // 2].tolist() and blob.onBorder == bool(shape["onBorder"][len(blobs) // 2])
        assert blob.extremeDensity == float(shape["extremeDensity"][len(blobs) // 2]) and blob.extremeCrs == shape["extremeCrs"][len(blobs) // 2].tolist()
        with pytest.raises(AttributeError):
            blob.anisotropy = 0.0
    assert count >= 20
    both = dm.createFullBlobLists(cut)
    joined = (both[0] + both[1]).shapeColumns()
    assert len(joined["anisotropy"]) == count and np.array_equal(joined["boxLo"][:len(both[0])], both[0].shapeColumns()["boxLo"])


def test_empty_repeated_freed_and_refused_lists(gpu_ctx):
    from pdb_eda_amd import _native
    header, grid, dm = device_map("orth", gpu_ctx)
    empty = dm._map.full_blobs(float(np.abs(grid).max()) * 2.0)
    assert len(empty) == 0
    got = empty.moments()
    assert all(len(got[k]) == 0 for k in MOMENT_COLUMNS) and got["s2"].shape == (0, 6)
    assert all(len(v) == 0 for v in dm.createFullBlobList(float(np.abs(grid).max()) * 2.0).shapeColumns().values())
    bl = dm._map.full_blobs(dm.meanDensity + 1.5 * dm.stdDensity)
    assert len(bl) >= 5 and bl.voxels()[0].shape[0] > 0
    gpu_ctx.profile_begin()
    first = bl.moments()
    launched = gpu_ctx.profile_end()
    assert {"k_blobshape_box", "k_blobshape_widths", "k_blobshape_sums", "k_blobshape_finish"} <= set(launched) and all(launched[k][0] == 1 for k in launched)
    gpu_ctx.profile_begin()
    second = bl.moments()
    assert gpu_ctx.profile_end() == {}                                       # a second call copies: no kernel
    assert_bytes_equal(second, first, "second call")
    bl.free()
    with pytest.raises(_native.PdbedaError):
        bl.moments()
    # a blob whose box is 2^15 voxels wide is refused in front of the moment launches, and the context stays usable
    row = np.zeros((1 << 15, 3), dtype=np.int32)
    row[:, 0] = np.arange(1 << 15)
    wide = dm._map.list_blobs(row)
    assert len(wide) == 1
    gpu_ctx.profile_begin()
    with pytest.raises(_native.PdbedaError) as refusal:
        wide.moments()
    launched = gpu_ctx.profile_end()
    assert refusal.value.code == _native.PDBEDA_ERR_ARGUMENT and "k_blobshape_sums" not in launched and "k_blobshape_box" in launched
    narrow = dm._map.list_blobs(row[: (1 << 15) - 1])
    got, want = assert_matches_checker(header, grid, narrow, False, "a row of 2^15 - 1 voxels")
    assert want["boxHi"].tolist() == [[(1 << 15) - 2, 0, 0]]
    assert_bytes_equal(dm._map.full_blobs(dm.meanDensity + 1.5 * dm.stdDensity).moments(), first, "after the refusal")


@pytest.fixture(scope="module", params=["orth", "hex"])
def analysis(request, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case(request.param)
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), request.param, ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), request.param, ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    return z, densityAnalysis.DensityAnalysis(request.param, dens, diff, st, pdb)


def check_shape_table(an, table, lists, std):
    """table: rows of blobShapeHeader for the blobs of ``lists`` (DeviceBlobs), in order."""
    atoms = np.asarray(an.symmetryAtomCoords, dtype=np.float64)
    ratio = an.densityElectronRatio
    at = 0
    for blobs in lists:
        shape, listed = blobs.shapeColumns(), blobs.columns()
        xyz = shape["extremeXyz"]
        d = np.sqrt(((xyz[:, None, :] - atoms[None, :, :]) ** 2).sum(axis=2))
        nearest = d.argmin(axis=1)
        for i in range(len(blobs)):
            row = table[at]
            at += 1
            assert row[0] == i and row[1] == int(listed["n"][i]) and row[2] == float(listed["volume"][i])
            assert row[3] == ("+" if listed["totalDensity"][i] >= 0 else "-") and row[4] == abs(float(listed["totalDensity"][i]) / ratio)
            assert row[5] == float(shape["extremeDensity"][i]) / std and row[6] == float(shape["extremeDensity"][i]) / ratio
            assert list(row[7]) == xyz[i].tolist() and [row[8], row[9], row[10]] == shape["principalLengths"][i].tolist()
            assert row[11] == float(shape["anisotropy"][i]) and list(row[12]) == shape["boxExtent"][i].tolist() and row[13] == bool(shape["onBorder"][i])
            assert abs(row[14] - d[i, nearest[i]]) <= 1e-9 and np.allclose(np.asarray(row[20], dtype=np.float64), atoms[nearest[i]], rtol=0, atol=1e-9)
    assert at == len(table)


def test_shape_table_and_mode(analysis, tmp_path):
    from pdb_eda_amd import densityAnalysis, singleStructure
    z, an = analysis
    diff, dens = an.diffDensityObj, an.densityObj
    header, table = singleStructure.rows(an, "shape", green=True, red=True)
    assert header == densityAnalysis.DensityAnalysis.blobShapeHeader and len(header) == 21
    cut = diff.meanDensity + 3.0 * diff.stdDensity
    lists = diff.createFullBlobLists(cut)
    assert len(lists[0]) >= 1 and len(lists[1]) >= 1 and len(table) == len(lists[0]) + len(lists[1])
    check_shape_table(an, table, lists, diff.stdDensity)
    for blobs in lists:
        stats = an.calculateBlobShapeStatistics(blobs)
        check_shape_table(an, stats, [blobs], diff.stdDensity)
    assert singleStructure.dumps(header, singleStructure.rows(an, "shape", green=True)[1] + singleStructure.rows(an, "shape", red=True)[1]) == singleStructure.dumps(header, table)
    blue = singleStructure.rows(an, "shape")[1]
    check_shape_table(an, blue, [dens.createFullBlobList(dens.meanDensity + 1.5 * dens.stdDensity)], dens.stdDensity)
    assert an.calculateBlobShapeStatistics(diff.createFullBlobList(float(np.abs(diff.density).max()) * 2.0)) == []
    with pytest.raises(ValueError):
        an.calculateBlobShapeStatistics(list(lists[0]))
    # both output formats through the existing writers
    back = json.loads(singleStructure.dumps(header, table, "json"))
    assert len(back) == len(table) and all(sorted(item) == sorted(header) for item in back)
    assert [item["anisotropy"] for item in back] == [row[11] for row in table] and [item["extreme_xyz"] for item in back] == [row[7] for row in table]
    path = tmp_path / "shape.csv"
    singleStructure.write(header, table, str(path), "csv")
    lines = list(csv.reader(open(str(path))))
    assert lines[0] == header and len(lines) == len(table) + 1
    # (a list cell is written as "[x, y, z]": three fields of the csv line, so principal_length_1 -- column 8 behind extreme_xyz -- is field 10)
    assert [int(line[0]) for line in lines[1:]] == [row[0] for row in table] and [float(line[10]) for line in lines[1:]] == [row[8] for row in table]
