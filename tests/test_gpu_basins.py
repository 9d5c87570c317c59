"""Peak basins on the MI355X path against tests/basins_checker.py, the plain numpy restatement of the contract in include/pdbeda.h
(pdbeda_peaklist_basins).  n, s1, neighbour, the basin volume and the bits of saddle are compared with np.array_equal over the whole
list; sum within 1e-9 n max |rho| (the bound of the partition and profile tests: the library rounds each voxel once to a quantum of
at most 2^-36 max |rho|, the checker's fp64 bincount errs by at most n^2 2^-53 max |rho|), sw1 within that bound times the largest
|d| of the basin.  The tile of the kernels is 64 x 8 x 8: the shapes below are the smallest that reach every path."""
import io

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import basins_checker

pytestmark = pytest.mark.gpu

COLUMNS = ("n", "sum", "s1", "sw1", "saddle", "neighbour")


def box_max(header, grid):
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    box = np.abs(np.asarray(grid, dtype=np.float64)[:us, :ur, :uc])
    return float(box[np.isfinite(box)].max())


def assert_basins(got, want, top, what=""):
    """got: PeakList.basins(volume=True);  want: basins_checker.find_basins();  top: max finite |rho| of the box."""
    print("%s: %d basins, %d significant voxels, %d orphans, longest ascent %d steps, %d rounds" %
          (what, len(want["n"]), want["significant"], want["orphans"], want["steps"], got["counters"]["rounds"]))
    assert np.array_equal(got["n"], want["n"]), what
    assert np.array_equal(got["s1"], want["s1"]), what
    assert np.array_equal(got["neighbour"], want["neighbour"]), what
    assert np.array_equal(got["saddle"].view(np.uint32), want["saddle"].view(np.uint32)), what
    assert np.array_equal(got["basin"], want["basin"]), what
    bound = 1e-9 * want["n"] * top
    err, err1 = np.abs(got["sum"] - want["sum"]), np.abs(got["sw1"] - want["sw1"]).max(axis=1) if len(want["n"]) else np.zeros(0)
    if len(want["n"]):
        print("%s: max |sum - checker| / bound = %.3g, max |sw1 - checker| / bound = %.3g" %
              (what, float((err / bound).max()), float((err1 / np.maximum(bound * want["maxd"], 1e-300)).max())))
    assert np.all(err <= bound), what
    assert np.all(err1 <= bound * want["maxd"]), what
    assert got["counters"]["significant"] == want["significant"] and got["counters"]["orphans"] == want["orphans"], what
    assert np.all(got["n"] >= 1)
    alone = want["n"] == 1
    assert not got["s1"][alone].any() and not got["sw1"][alone].any()          # exact zeros


def same_columns(a, b, volume=True):
    keys = COLUMNS + (("basin",) if volume else ())
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in keys)


def make_dm(gpu_ctx, shape, seed, sigma_voxels=1.5, quantum=None, name="basins", edit=None):
    from pdb_eda_amd import ccp4, synthetic
    spec = synthetic.MapSpec(ncrs=shape, spacing=0.5)
    grid = synthetic.noise_grid(spec, seed, sigma_voxels)
    if quantum is not None:         # steps of `quantum` standard deviations: exact ties abound
        step = np.float32(quantum * float(np.std(grid.astype(np.float64))))
        grid = (np.rint(grid / step) * step).astype(np.float32)
    if edit is not None:
        grid = edit(grid)
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=gpu_ctx), grid


def dm_of_grid(gpu_ctx, grid, name):
    """grid: float32 [ns][nr][nc]."""
    from pdb_eda_amd import ccp4, synthetic
    spec = synthetic.MapSpec(ncrs=(grid.shape[2], grid.shape[1], grid.shape[0]), spacing=0.5)
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=gpu_ctx)


# ---- the voxel goldens ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=VOXEL_CASES)
def case(request, gpu_ctx):
    from pdb_eda_amd import ccp4
    z, header, grid = load_case(request.param)
    dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), request.param, ctx=gpu_ctx)
    return request.param, header, grid, dm


@pytest.mark.parametrize("nsd", [1.5, -1.5, 3.0, -3.0])
def test_golden_maps_against_checker(case, nsd):
    name, header, grid, dm = case
    cut = (1 if nsd > 0 else -1) * (dm.meanDensity + abs(nsd) * dm.stdDensity)
    pl = dm._map.peaks(cut)
    want = basins_checker.find_basins(header, grid, cut)
    assert len(pl) == len(want["n"]) and want["orphans"] == 0
    assert_basins(pl.basins(volume=True), want, box_max(header, grid), "%s %+g sigma" % (name, nsd))
    # the Python surface: the finished columns, and the same values as attributes of the peaks
    peaks = dm.findPeaks(cut)
    cols = peaks.basinColumns()
    assert np.array_equal(cols["numVoxels"], want["n"]) and np.array_equal(cols["neighbour"], want["neighbour"])
    assert np.array_equal(peaks.basinVolume(), want["basin"])
    if len(peaks):
        last = len(peaks) - 1
        assert peaks[0].numVoxels == int(want["n"][0]) and peaks[last].neighbour == int(want["neighbour"][last])
        assert peaks[last].prominence == float(cols["prominence"][last]) and list(peaks[0].centroid) == cols["centroid"][0].tolist()
        whole = want["neighbour"] == -1
        assert np.all(cols["saddle"][whole] == np.float32(cut))
        assert np.all(cols["prominence"] >= 0)


# ---- long ascents: a serpentine through every tile border ----------------------------------------------------------------
def serpentine(shape=(130, 20, 20)):
    """Voxels (c, r, s) of one path: rows along c at r = 0, 2, 4, ..., joined at alternating ends by single voxels at odd r; the same
    on the planes s = 0, 2, ..., joined by single voxels at odd s.  The gaps keep the rows and planes from touching anywhere else."""
    nc, nr, ns = shape
    path = []
    rows = list(range(0, nr, 2))
    forward = True                         # along c
    upward = True                          # along r
    for s in range(0, ns, 2):
        if path:
            path.append((path[-1][0], path[-1][1], s - 1))
        for k, r in enumerate(rows if upward else rows[::-1]):
            if k:
                path.append((path[-1][0], (r - 1) if upward else (r + 1), s))
            path.extend((c, r, s) for c in (range(nc) if forward else range(nc - 1, -1, -1)))
            forward = not forward
        upward = not upward
    assert len(set(path)) == len(path)
    return path


def serpentine_grid(values, shape=(130, 20, 20)):
    path = np.array(serpentine(shape))
    grid = np.zeros((shape[2], shape[1], shape[0]), dtype=np.float32)
    grid[path[:, 2], path[:, 1], path[:, 0]] = values(len(path)).astype(np.float32)
    return grid, path


def test_long_ascent_is_one_basin(gpu_ctx):
    grid, path = serpentine_grid(lambda n: 1.0 + 1e-3 * np.arange(n))
    dm = dm_of_grid(gpu_ctx, grid, "serpentine")
    want = basins_checker.find_basins(dm.header, grid, 0.5)
    assert len(want["n"]) == 1 and want["n"][0] == len(path) > 13000 and want["steps"] > 1000
    assert want["peaks"]["crs"][0].tolist() == list(path[-1]) and want["neighbour"].tolist() == [-1]
    pl = dm._map.peaks(0.5)
    got = pl.basins(volume=True)
    assert_basins(got, want, box_max(dm.header, grid), "serpentine")
    assert 2 <= got["counters"]["rounds"] <= 31
    assert got["counters"]["arena_bytes"] >= 4 * grid.size


def test_serpentine_with_two_summits(gpu_ctx):
    def values(n):
        k = np.arange(n, dtype=np.float64)
        k1, km, k2 = n // 4, n // 2 + 40, 3 * n // 4          # (km: mid-row, so its two path neighbours are no neighbours of each other)
        v = np.where(k <= k1, 1.0 + 1e-3 * k, np.where(k <= km, 1.0 + 1e-3 * k1 - 1e-3 * (k - k1), 0.0))
        valley = 1.0 + 1e-3 * k1 - 1e-3 * (km - k1)
        v = np.where(k > km, np.where(k <= k2, valley + 1.5e-3 * (k - km), valley + 1.5e-3 * (k2 - km) - 1e-3 * (k - k2)), v)
        return v
    grid, path = serpentine_grid(values)
    n = len(path)
    km = n // 2 + 40
    assert 2 < path[km][0] < 127 and path[km - 1][1:].tolist() == path[km + 1][1:].tolist()
    dm = dm_of_grid(gpu_ctx, grid, "two summits")
    cut = 0.5
    assert float(grid[grid > 0].min()) > cut
    want = basins_checker.find_basins(dm.header, grid, cut)
    pass_value = grid[path[km][2], path[km][1], path[km][0]]
    assert len(want["n"]) == 2 and int(want["n"].sum()) == n
    assert want["saddle"].tolist() == [float(pass_value)] * 2 and want["neighbour"].tolist() == [1, 0]
    assert want["peaks"]["crs"].tolist() == [list(path[3 * n // 4]), list(path[n // 4])]
    green = dm._map.full_blobs(cut)
    assert len(green) == 1                                     # two basins, ONE blob
    got = dm._map.peaks(cut, green).basins(volume=True)
    assert_basins(got, want, box_max(dm.header, grid), "two summits")
    assert 2 <= got["counters"]["rounds"] <= 31


def test_plateau_is_one_basin(gpu_ctx):
    grid = np.full((9, 9, 70), 2.0, dtype=np.float32)
    dm = dm_of_grid(gpu_ctx, grid, "plateau")
    want = basins_checker.find_basins(dm.header, grid, 1.0)
    assert want["peaks"]["crs"].tolist() == [[0, 0, 0]] and want["n"].tolist() == [70 * 9 * 9] and want["neighbour"].tolist() == [-1]
    got = dm._map.peaks(1.0).basins(volume=True)
    assert_basins(got, want, 2.0, "plateau")
    assert got["saddle"].tolist() == [0.0] and not got["basin"].any()
    assert got["s1"].tolist() == [[9 * 9 * (69 * 70 // 2), 70 * 9 * (8 * 9 // 2), 70 * 9 * (8 * 9 // 2)]]


# ---- ties: the single list, the fused lists and the checker ----------------------------------------------------------------
@pytest.fixture(scope="module")
def smooth(gpu_ctx):
    return make_dm(gpu_ctx, (96, 72, 80), seed=7)


@pytest.fixture(scope="module")
def quantised(gpu_ctx):
    return make_dm(gpu_ctx, (96, 72, 80), seed=7, quantum=0.25)


def test_quantised_map_single_fused_and_checker(quantised):
    dm, grid = quantised
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    fpos, fneg = dm._map.peaks_pm(cut, -cut)
    top = box_max(dm.header, grid)
    for fused, c in ((fpos, cut), (fneg, -cut)):
        want = basins_checker.find_basins(dm.header, grid, c)
        ties = len(want["peaks"]["height"]) - len(np.unique(want["peaks"]["height"]))
        print("peaks that share their height with another: %d" % ties)
        assert ties > 0
        single = dm._map.peaks(c).basins(volume=True)
        assert_basins(single, want, top, "quantised %+.3g" % c)
        assert same_columns(single, fused.basins(volume=True))              # the fused call equals the single call to the bit


# ---- basins and blobs agree --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsd", [1.5, 3.0])
def test_basins_agree_with_blobs(smooth, nsd):
    dm, grid = smooth
    cut = dm.meanDensity + nsd * dm.stdDensity
    green, red = dm._map.full_blobs_pm(cut, -cut, labels=True)
    pos, neg = dm._map.peaks_pm(cut, -cut, green, red)
    top = box_max(dm.header, grid)
    for peaks, blobs in ((pos, green), (neg, red)):
        rows, got, stats = peaks.rows(), peaks.basins(volume=True), blobs.stats()
        labels = blobs.labels(dm._map.unique_shape)
        n_blobs, blob, crs, basin = len(blobs), rows["blob"], rows["crs"], got["basin"]
        print("%d basins in %d blobs at %g sigma" % (len(crs), n_blobs, nsd))
        assert n_blobs > 1 and len(crs) > n_blobs
        assert np.array_equal(np.bincount(blob, weights=got["n"], minlength=n_blobs).astype(np.int64), stats["n"])
        assert np.all(np.abs(np.bincount(blob, weights=got["sum"], minlength=n_blobs) - stats["totalDensity"]) <= 1e-9 * stats["n"] * top)
        assert np.array_equal(basin[crs[:, 2], crs[:, 1], crs[:, 0]], np.arange(len(crs)))
        inside = basin >= 0
        assert np.array_equal(labels[inside], blob[basin[inside]]) and np.array_equal(inside, labels >= 0)
        assert np.array_equal(got["neighbour"] == -1, np.bincount(blob, minlength=n_blobs)[blob] == 1)
        linked = got["neighbour"] >= 0
        assert np.all(np.abs(got["saddle"][got["neighbour"][linked]]) >= np.abs(got["saddle"][linked]))
        assert np.all(blob[got["neighbour"][linked]] == blob[linked])       # the basin beyond the pass lies in the same blob


# ---- a wider grid: two tiles and more on every axis, twelve along s ----------------------------------------------------------
def test_wider_grid_against_checker(gpu_ctx):
    dm, grid = make_dm(gpu_ctx, (160, 128, 96), seed=13)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    want = basins_checker.find_basins(dm.header, grid, cut)
    assert_basins(dm._map.peaks(cut).basins(volume=True), want, box_max(dm.header, grid), "160 x 128 x 96")


# ---- NaN and +inf ------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_voxels(gpu_ctx):
    from pdb_eda_amd import synthetic
    shape = (20, 12, 10)
    clean = synthetic.noise_grid(synthetic.MapSpec(ncrs=shape, spacing=0.5), 21, 1.5)
    cut = float(np.mean(clean, dtype=np.float64) + 1.0 * np.std(clean.astype(np.float64)))
    order = np.argsort(clean, axis=None)[::-1]
    top_s, top_r, top_c = np.unravel_index(order[0], clean.shape)

    def edit(grid):
        grid = grid.copy()
        # a NaN beside the highest voxel: that voxel stays a root and is no peak any more -- its basin is orphaned
        grid[top_s, top_r, top_c + 1 if top_c + 1 < shape[0] else top_c - 1] = np.nan
        lowest = np.unravel_index(order[-1], clean.shape)
        grid[lowest] = np.nan                                   # a NaN among the insignificant (for +cut) voxels
        far = [i for i in order[:200] if abs(np.unravel_index(i, clean.shape)[2] - top_c) > 4 and clean.flat[i] > cut]
        grid[np.unravel_index(far[len(far) // 2], clean.shape)] = np.inf      # a significant voxel becomes +inf: counted, in no sum
        return grid
    dm, grid = make_dm(gpu_ctx, shape, seed=21, edit=edit)
    assert np.isnan(grid).sum() == 2 and np.isinf(grid).sum() == 1
    for c in (cut, -cut):
        want = basins_checker.find_basins(dm.header, grid, c)
        got = dm._map.peaks(c).basins(volume=True)
        assert_basins(got, want, box_max(dm.header, grid), "NaN / inf %+.3g" % c)
        assert np.all(np.isfinite(got["sum"])) and np.all(np.isfinite(got["sw1"]))
        if c > 0:
            assert want["orphans"] > 0 and got["basin"][top_s, top_r, top_c] == -1
            assert np.isinf(want["peaks"]["height"][0])


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_two_fresh_lists_are_byte_equal(quantised):
    dm, _ = quantised
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    for c in (cut, -cut):
        a, b = dm._map.peaks(c).basins(volume=True), dm._map.peaks(c).basins(volume=True)
        assert len(a["n"]) > 0 and same_columns(a, b) and a["counters"] == b["counters"]


# ---- errors and the kept rows --------------------------------------------------------------------------------------------------
def test_empty_list_freed_list_and_kept_rows(gpu_ctx, smooth):
    from pdb_eda_amd import _native
    dm, grid = smooth
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    empty = dm._map.peaks(float(np.abs(grid).max()) * 2.0)
    assert len(empty) == 0
    got = empty.basins(volume=True)
    assert all(len(got[k]) == 0 for k in COLUMNS) and np.all(got["basin"] == -1) and got["basin"].shape == dm._map.unique_shape
    assert got["counters"] == {"significant": 0, "orphans": 0, "rounds": 0, "arena_bytes": 0}
    # the kept rows: a second call launches nothing
    pl = dm._map.peaks(cut)
    first = pl.basins()
    gpu_ctx.profile_begin()
    second = pl.basins()
    assert not [name for name in gpu_ctx.profile_end() if name.startswith("k_")]
    assert same_columns(first, second, volume=False) and first["counters"] == second["counters"] and first["counters"]["rounds"] >= 1
    # a freed list and a NULL list are refused before any launch; the context lives
    lib = _native.lib()
    assert lib.pdbeda_peaklist_basins(None, None, None, None, None, None, None, None, None) == _native.PDBEDA_ERR_ARGUMENT
    pl.free()
    with pytest.raises(_native.PdbedaError):
        pl.basins()
    again = dm._map.peaks(cut).basins()
    assert same_columns(first, again, volume=False)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def test_basin_statistics_and_single_structure_table(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis, singleStructure
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    an = densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb)
    header, table = singleStructure.rows(an, "basin", green=True, red=True)
    assert header == densityAnalysis.DensityAnalysis.basinStatisticsHeader and len(header) == 21
    peak_header, peak_table = singleStructure.rows(an, "peak", green=True, red=True)
    assert len(table) == len(peak_table) > 0
    assert singleStructure.dumps(peak_header, [row[:13] for row in table]) == singleStructure.dumps(peak_header, peak_table)      # the shared columns
    _, blob_table = singleStructure.rows(an, "blob", green=True, red=True)
    for sign in "+-":
        blob_electrons = np.array([row[2] for row in blob_table if row[1] == sign])
        mine = [row for row in table if row[1] == sign]
        index = np.array([row[4] for row in mine])
        electrons = np.bincount(index, weights=[row[15] for row in mine], minlength=len(blob_electrons))
        print("%s: %d basins in %d blobs, max |sum of electrons - blob table| = %.3g" % (sign, len(mine), len(blob_electrons), float(np.abs(electrons - blob_electrons).max())))
        assert np.all(np.abs(electrons - blob_electrons) <= 1e-8)
        fraction = np.bincount(index, weights=[row[16] for row in mine], minlength=len(blob_electrons))
        assert np.allclose(fraction, 1.0, rtol=0, atol=1e-9)
    for peaks in (an.greenPeakList, an.redPeakList):
        stats = an.calculateAtomSpecificBasinStatistics(peaks)
        cols = peaks.basinColumns()
        assert [row[13] for row in stats] == cols["numVoxels"].tolist() and [row[19] for row in stats] == cols["neighbour"].tolist()
        assert np.allclose([row[18] for row in stats], cols["prominence"] / diff.stdDensity, rtol=1e-12, atol=0)
        grouped = ccp4.groupBasins(cols, 0.5 * diff.stdDensity)
        assert int(grouped["numVoxels"].sum()) == int(cols["numVoxels"].sum()) and len(grouped["groups"]) <= len(stats)
    # blue comes from the 2Fo-Fc map, and the writers take the table
    blue_header, blue = singleStructure.rows(an, "basin")
    assert len(blue) == len(singleStructure.rows(an, "peak")[1]) > 0
    assert singleStructure.dumps(blue_header, blue, "json") and singleStructure.dumps(blue_header, blue, "csv")
    assert an.calculateAtomSpecificBasinStatistics([]) == []
