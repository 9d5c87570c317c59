"""Density peak search on the MI355X path against tests/peaks_checker.py, the plain numpy restatement of the contract in
include/pdbeda.h (pdbeda_map_peaks).  crs, height, on_border and the order of the list are compared with np.array_equal over
the whole list; refined_xyz within 1e-9 A and refined_height within 1e-12 relative (fp64 derived values)."""
import csv
import io
import json

import numpy as np
import pytest

from conftest import VOXEL_CASES, load_analysis_case, load_case
import peaks_checker

pytestmark = pytest.mark.gpu


def assert_rows_equal(got, want, what=""):
    """got: PeakList.rows();  want: peaks_checker.find_peaks()."""
    print("%s: %d peaks (checker %d)" % (what, len(got["crs"]), len(want["crs"])))
    assert np.array_equal(got["crs"], want["crs"]), what
    assert np.array_equal(got["height"].view(np.uint32), want["height"].view(np.uint32)), what
    assert np.array_equal(got["onBorder"], want["on_border"]), what
    if len(want["crs"]):
        dx = float(np.abs(got["xyz"] - want["refined_xyz"]).max())
        scale = np.abs(want["refined_height"])
        dh = float((np.abs(got["refinedHeight"] - want["refined_height"]) / np.where(scale > 0, scale, 1.0)).max())
        print("%s: max |xyz - checker| = %.3g A, max relative refined-height error = %.3g" % (what, dx, dh))
        assert dx <= 1e-9, what
        assert np.all(np.abs(got["refinedHeight"] - want["refined_height"]) <= 1e-12 * scale), what


def same_rows(a, b):
    return all(np.array_equal(a[k].view(np.uint8) if a[k].dtype.kind == "f" else a[k], b[k].view(np.uint8) if b[k].dtype.kind == "f" else b[k]) for k in a)


def make_dm(gpu_ctx, shape, seed, sigma_voxels=1.5, quantum=None, name="peaks"):
    from pdb_eda_amd import ccp4, synthetic
    spec = synthetic.MapSpec(ncrs=shape, spacing=0.5)
    grid = synthetic.noise_grid(spec, seed, sigma_voxels)
    if quantum is not None:         # steps of `quantum` standard deviations: exact ties by the million
        step = np.float32(quantum * float(np.std(grid.astype(np.float64))))
        grid = (np.rint(grid / step) * step).astype(np.float32)
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
    want = peaks_checker.find_peaks(header, grid, cut)
    assert len(pl) == len(want["crs"])
    got = pl.rows()
    assert_rows_equal(got, want, "%s %+g sigma" % (name, nsd))
    assert np.all(got["blob"] == -1)
    ctr = pl.counters()
    with np.errstate(invalid="ignore"):
        box = grid[:header.uniqueNcrs[2], :header.uniqueNcrs[1], :header.uniqueNcrs[0]]
        assert ctr["tested"] == int(np.count_nonzero(box >= np.float32(cut) if cut > 0 else box <= np.float32(cut)))
    assert ctr["peaks"] == len(want["crs"])
    # the Python surface: the same list as DensityPeak items
    peaks = dm.findPeaks(cut)
    assert len(peaks) == len(want["crs"])
    if len(peaks):
        assert list(peaks[0].crs) == want["crs"][0].tolist() and peaks[0].height == float(want["height"][0]) and peaks[0].blobIndex == -1
        assert peaks[len(peaks) - 1].onBorder == bool(want["on_border"][-1])
    assert dm.findPeaks(0.0) is None


# ---- 256^3: smooth noise, and the same map in steps of a quarter sigma (ties) --------------------------------------------
@pytest.mark.parametrize("quantum", [None, 0.25], ids=["smooth", "quantised"])
def test_256_cubed_single_and_fused(gpu_ctx, quantum):
    dm = make_dm(gpu_ctx, (256, 256, 256), seed=11, quantum=quantum)
    header, grid = dm.header, dm.density
    for nsd in (1.5, 3.0):
        cut = dm.meanDensity + nsd * dm.stdDensity
        pos, neg = dm._map.peaks(cut), dm._map.peaks(-cut)
        fpos, fneg = dm._map.peaks_pm(cut, -cut)
        for single, fused, c in ((pos, fpos, cut), (neg, fneg, -cut)):
            want = peaks_checker.find_peaks(header, grid, c)
            assert_rows_equal(single.rows(), want, "256^3 %s %+g sigma" % ("quantised" if quantum else "smooth", nsd if c > 0 else -nsd))
            assert same_rows(single.rows(), fused.rows())           # the fused call equals two single calls to the bit
            if quantum:
                ties = len(want["height"]) - len(np.unique(want["height"]))
                print("peaks that share their height with another: %d" % ties)
                assert ties > 0
        assert not (set(map(tuple, fpos.rows()["crs"].tolist())) & set(map(tuple, fneg.rows()["crs"].tolist())))    # green and red are disjoint


# ---- peaks and blobs agree -------------------------------------------------------------------------------------------------
def check_blob_invariants(dm, peaks, blobs, cut, what):
    rows = peaks.rows()
    labels = blobs.labels(dm._map.unique_shape)                       # [us][ur][uc], blob index or -1
    crs = rows["crs"]
    n_blobs = len(blobs)
    print("%s: %d peaks in %d blobs" % (what, len(crs), n_blobs))
    assert len(crs) >= n_blobs
    assert np.array_equal(rows["blob"], labels[crs[:, 2], crs[:, 1], crs[:, 0]]) and np.all(rows["blob"] >= 0)
    # every blob holds a peak, and its first peak in list order is its extreme voxel under the order of the contract
    first = np.full(n_blobs, -1, dtype=np.int64)
    for i in range(len(crs) - 1, -1, -1):
        first[rows["blob"][i]] = i
    assert np.all(first >= 0)
    vox, off = blobs.voxels()
    density = dm.density
    ur, us = dm.header.uniqueNcrs[1], dm.header.uniqueNcrs[2]
    for b in range(n_blobs):
        v = vox[off[b]:off[b + 1]].astype(np.int64)
        d = density[v[:, 2], v[:, 1], v[:, 0]].astype(np.float64)
        key = (v[:, 0] * ur + v[:, 1]) * us + v[:, 2]
        best = np.lexsort((key, -d if cut > 0 else d))[0]
        assert v[best].tolist() == crs[first[b]].tolist(), (what, b)


@pytest.mark.parametrize("name", ["orth", "hex", "orth_rep", "wide", "noise"])
def test_peaks_agree_with_blobs(gpu_ctx, name):
    from pdb_eda_amd import ccp4
    if name == "noise":
        dm = make_dm(gpu_ctx, (200, 96, 80), seed=5)
    else:
        z, _, _ = load_case(name)
        dm = ccp4.parse(io.BytesIO(z["ccp4_bytes"].tobytes()), name, ctx=gpu_ctx)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    for with_labels in (True, False):        # the list's own label volume, or one the peak job makes for itself
        green, red = dm._map.full_blobs_pm(cut, -cut, labels=with_labels)
        pos, neg = dm._map.peaks_pm(cut, -cut, green, red)
        check_blob_invariants(dm, pos, green, cut, "%s green fused" % name)
        check_blob_invariants(dm, neg, red, -cut, "%s red fused" % name)
        lone = dm._map.full_blobs(-cut, labels=with_labels)
        check_blob_invariants(dm, dm._map.peaks(-cut, lone), lone, -cut, "%s red alone" % name)
        only_green = dm._map.peaks_pm(cut, -cut, green, None)
        assert np.array_equal(only_green[0].rows()["blob"], pos.rows()["blob"]) and np.all(only_green[1].rows()["blob"] == -1)
    # the Python surface
    blobs = dm.createFullBlobList(cut)
    peaks = dm.findPeaks(cut, blobs)
    assert np.array_equal(peaks.columns()["blobIndex"], pos.rows()["blob"])
    pair = dm.findPeakLists(cut, dm.createFullBlobLists(cut))
    assert np.array_equal(pair[1].columns()["blobIndex"], neg.rows()["blob"])


# ---- determinism, arena overflow -------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(gpu_ctx):
    dm = make_dm(gpu_ctx, (192, 128, 96), seed=2, quantum=0.25)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    green, red = dm._map.full_blobs_pm(cut, -cut)
    calls = [lambda: [dm._map.peaks(cut)], lambda: [dm._map.peaks(-cut)], lambda: list(dm._map.peaks_pm(cut, -cut)),
             lambda: list(dm._map.peaks_pm(cut, -cut, green, red)), lambda: [dm._map.peaks(cut, green)]]
    for call in calls:
        a, b = call(), call()
        for x, y in zip(a, b):
            assert len(x) > 0 and same_rows(x.rows(), y.rows())


def test_arena_overflow_runs_the_job_again(gpu_ctx):
    """White noise has a local maximum per 27 voxels, the typical-size arena holds one per 64: the job must run twice and
    return the checker's list all the same."""
    for nsd in (0.5, 0.25, 0.0625):          # (a denser map if the first did not overflow)
        dm = make_dm(gpu_ctx, (128, 128, 128), seed=9, sigma_voxels=0)
        cut = dm.meanDensity + nsd * dm.stdDensity
        pl = dm._map.peaks(cut)
        ctr = pl.counters()
        print("white noise 128^3 at %g sigma: %r" % (nsd, ctr))
        if ctr["reruns"] >= 1:
            break
    assert ctr["reruns"] == 1
    want = peaks_checker.find_peaks(dm.header, dm.density, cut)
    assert_rows_equal(pl.rows(), want, "white noise %g sigma" % nsd)
    fpos, fneg = dm._map.peaks_pm(cut, -cut)
    assert fpos.counters()["reruns"] == 1 and same_rows(fpos.rows(), pl.rows())
    assert_rows_equal(fneg.rows(), peaks_checker.find_peaks(dm.header, dm.density, -cut), "white noise -%g sigma" % nsd)


# ---- the tables ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["orth", "hex"])
def analysis(request, gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case(request.param)
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), request.param, ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), request.param, ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    return z, densityAnalysis.DensityAnalysis(request.param, dens, diff, st, pdb)


def nearest_atoms(xyz, atoms):
    d = np.sqrt(((xyz[:, None, :] - atoms[None, :, :]) ** 2).sum(axis=2))
    idx = d.argmin(axis=1)
    return idx, d[np.arange(len(xyz)), idx]


def check_peak_table(an, table, wants, dm_std):
    want_xyz = np.concatenate([w["refined_xyz"] for w in wants])
    want_height = np.concatenate([w["height"] for w in wants]).astype(np.float64)
    assert len(table) == len(want_xyz) and len(table) > 0
    atoms = np.asarray(an.symmetryAtomCoords, dtype=np.float64)
    idx, dist = nearest_atoms(want_xyz, atoms)
    got_dist = np.array([row[0] for row in table])
    print("peak table: %d rows, max |distance - numpy| = %.3g" % (len(table), float(np.abs(got_dist - dist).max())))
    assert np.all(np.abs(got_dist - dist) <= 1e-9)
    assert np.all(np.abs(np.array([list(row[11]) for row in table]) - atoms[idx]) <= 1e-9)       # the atom
    assert np.all(np.abs(np.array([list(row[12]) for row in table]) - want_xyz) <= 1e-9)          # the peak
    sym = an.symmetryAtoms
    for row, i in zip(table, idx.tolist()):
        atom = sym[i]
        assert (row[6], row[7], row[8], row[9], tuple(row[10])) == (atom.parent.parent.id, atom.parent.id[1], atom.parent.resname, atom.name, tuple(atom.symmetry))
    assert [row[1] for row in table] == ["+" if h >= 0 else "-" for h in want_height]
    assert np.allclose([row[2] for row in table], want_height / dm_std, rtol=1e-12, atol=0)
    assert np.allclose([row[3] for row in table], want_height / an.densityElectronRatio, rtol=1e-12, atol=0)


def test_peak_statistics_and_single_structure_table(analysis, tmp_path):
    from pdb_eda_amd import densityAnalysis, singleStructure
    z, an = analysis
    diff = an.diffDensityObj
    cut = diff.diffDensityCutoff
    wants = [peaks_checker.find_peaks(diff.header, diff.density, cut), peaks_checker.find_peaks(diff.header, diff.density, -cut)]
    header, table = singleStructure.rows(an, "peak", green=True, red=True)              # asked for first: the blob table below must not notice
    assert header == densityAnalysis.DensityAnalysis.peakStatisticsHeader and len(header) == 13
    check_peak_table(an, table, wants, diff.stdDensity)
    for peaks, want in ((an.greenPeakList, wants[0]), (an.redPeakList, wants[1])):
        stats = an.calculateAtomSpecificPeakStatistics(peaks)
        check_peak_table(an, stats, [want], diff.stdDensity)
        assert [row[4] for row in stats] == peaks.columns()["blobIndex"].tolist() and min(row[4] for row in stats) >= 0
        assert [row[5] for row in stats] == want["on_border"].tolist()
        hdr = densityAnalysis.DensityAnalysis.peakStatisticsHeader
        assert singleStructure.dumps(hdr, an.calculateAtomSpecificPeakStatistics(list(peaks))) == singleStructure.dumps(hdr, stats)    # a plain list of the same peaks
    # the two halves of the fused table are the single-colour tables, and blue comes from the 2Fo-Fc map
    assert singleStructure.dumps(header, singleStructure.rows(an, "peak", green=True)[1] + singleStructure.rows(an, "peak", red=True)[1]) == singleStructure.dumps(header, table)
    dens = an.densityObj
    blue_cut = dens.meanDensity + 1.5 * dens.stdDensity
    check_peak_table(an, singleStructure.rows(an, "peak")[1], [peaks_checker.find_peaks(dens.header, dens.density, blue_cut)], dens.stdDensity)
    assert len(an.bluePeakList) == len(peaks_checker.find_peaks(dens.header, dens.density, dens.densityCutoff)["crs"])
    # writers round-trip
    back = json.loads(singleStructure.dumps(header, table, "json"))
    assert len(back) == len(table) and all(sorted(item) == sorted(header) for item in back)
    assert [item["distance_to_atom"] for item in back] == [row[0] for row in table] and [item["peak_xyz"] for item in back] == [row[12] for row in table]
    path = tmp_path / "peaks.csv"
    singleStructure.write(header, table, str(path), "csv")
    lines = list(csv.reader(open(str(path))))
    assert lines[0] == header and len(lines) == len(table) + 1
    assert [float(line[0]) for line in lines[1:]] == [row[0] for row in table]
    # the existing blob table of the same analyzer is what a fresh analyzer gives
    from pdb_eda_amd import ccp4, synthetic
    _, spec, st, pdb, params = load_analysis_case(an.pdbid)
    dens2 = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), an.pdbid, ctx=dens._ctx)
    diff2 = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), an.pdbid, ctx=dens._ctx)
    densityAnalysis._attachCutoffs(dens2, diff2)
    fresh = densityAnalysis.DensityAnalysis(an.pdbid, dens2, diff2, st, pdb)
    for colours in ({"green": True, "red": True}, {}):
        assert singleStructure.dumps(*singleStructure.rows(an, "blob", **colours)) == singleStructure.dumps(*singleStructure.rows(fresh, "blob", **colours))


def test_peak_statistics_fail_like_the_blob_table(gpu_ctx):
    """No operators -> no symmetry atoms -> the blob table's ValueError; no ratio -> its RuntimeError."""
    import copy
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    bare = copy.deepcopy(pdb)
    bare.header.rotationMats = []
    an = densityAnalysis.DensityAnalysis("orth", dens, diff, st, bare)
    assert an.greenPeakList and an.calculateAtomSpecificPeakStatistics([]) == []
    with pytest.raises(ValueError):
        an.calculateAtomSpecificPeakStatistics(an.greenPeakList)
    an2 = densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb)
    an2.aggregateCloud = lambda *a, **k: None
    with pytest.raises(RuntimeError):
        an2.calculateAtomSpecificPeakStatistics(an2.greenPeakList)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_context_lives(gpu_ctx):
    from pdb_eda_amd import _native
    dm = make_dm(gpu_ctx, (70, 40, 36), seed=3)
    other = make_dm(gpu_ctx, (70, 40, 36), seed=4)
    cut = dm.meanDensity + 1.5 * dm.stdDensity
    before = dm._map.peaks(cut).rows()
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks(0.0)
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks_pm(cut, cut)
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks(cut, other._map.full_blobs(cut))              # a list of another map
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks(cut, dm._map.full_blobs(cut * 1.25))          # ... of another cutoff
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks(cut, dm._map.full_blobs(-cut))                # ... of the other sign
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks_pm(cut, -cut, None, dm._map.full_blobs(cut))
    sphere = dm._map.sphere_blobs(np.array([[5.0, 5.0, 5.0]]), np.array([2.0], dtype=np.float32), np.array([0, 1], dtype=np.int64), cut)
    with pytest.raises(_native.PdbedaError):
        dm._map.peaks(cut, sphere)                                   # not a whole-map list
    # the context is usable afterwards and gives what it gave before
    assert same_rows(dm._map.peaks(cut).rows(), before)
    assert len(dm._map.full_blobs(cut)) > 0 and dm.meanDensity == dm._map.stats()[0]
