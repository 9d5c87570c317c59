"""The reciprocal-space calls on the MI355X path (pdbeda_map_fft, pdbeda_spectrum_inverse / _scale / _shells / _values and the Python on top of them)
against tests/fourier_checker.py, the numpy restatement of the contracts in include/pdbeda.h, and -- TO THE BIT -- against tests/fourier_harness.cpp,
the host build of the line transform the kernels run (pdb_eda_amd/csrc/pdbeda_fourier_line.h: same source, same -ffp-contract=off, IEEE fp64).
tests/test_fourier_host.py holds the harness and the checker themselves against numpy."""
import ctypes
import io

import numpy as np
import pytest

from conftest import load_analysis_case
import fourier_cases as fc
import fourier_checker as ck

pytestmark = pytest.mark.gpu

_maps, _wanted = {}, {}


def device_map(name, gpu_ctx, grid=None, tag="a"):
    """A DensityMatrix on the geometry ``name`` holding ``grid`` (default: the seeded map of that geometry), and the grid."""
    from pdb_eda_amd import ccp4, synthetic
    key = (name, tag)
    if key not in _maps:
        data = fc.grid_of(name) if grid is None else grid
        _maps[key] = (ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(fc.spec_of(name), data)), name, ctx=gpu_ctx), np.array(data, dtype=np.float32))
    return _maps[key]


def second_map(name, gpu_ctx):
    return device_map(name, gpu_ctx, fc.grid_of(name, seed=1, offset=-0.5), tag="b")


def wanted(key, make):
    """A reference, computed once per case and shared (never modified)."""
    if key not in _wanted:
        _wanted[key] = make()
    return _wanted[key]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("fourier")
    return fc.build_harness(d, sanitize=False), d


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_work_units_are_the_kernels():
    text = open(fc.os.path.join(fc.CSRC, "pdbeda_fourier.h")).read()
    assert "constexpr int FFT_LINES = %d;" % fc.T in text and fc.T == fc.R
    assert "#define PDBEDA_FFT_MAX_AXIS %d" % fc.MAX_AXIS in open(fc.os.path.join(fc.CSRC, "pdbeda_fourier_line.h")).read()


# ---- the forward transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.FORWARD)
def test_forward_against_checker_and_harness(gpu_ctx, harness, name):
    """Relative L2 error against numpy within 16 eps max(1, log2 N); equal TO THE BIT to the host build of the same line code; two calls agree
    to the bit."""
    exe, d = harness
    dm, grid = device_map(name, gpu_ctx)
    spec = dm.fourier()
    assert spec.shape == (grid.shape[0], grid.shape[1], grid.shape[2] // 2 + 1)
    got = spec.values()
    want = wanted(("rfftn", name), lambda: ck.forward(grid))
    err, bound = ck.rel_l2(got, want), ck.forward_bound(grid.shape)
    print("%s: relative L2 error %.3g, bound %.3g" % (name, err, bound))
    assert err <= bound
    host = wanted(("harness", name), lambda: fc.harness_volume(exe, d, grid, name))
    assert same_bits(got, host), "%s: %d of %d coefficients differ from the host build" % (name, int((got != host).sum()), got.size)
    assert same_bits(dm.fourier().values(), got)
    assert float(np.abs(got).max()) > 0.1          # (a vacuous comparison cannot pass)


def test_position_in_a_tile_changes_no_bit(gpu_ctx, harness):
    """A map whose 32 rows all hold ONE line of 30 (radices 2, 3, 5), 8 x 4 rows: were the row spectra after the pass along c not bit-identical,
    the passes along r and s -- radix 2 and 4 on CONSTANT lines, which are exact: sums of equal numbers and exact zeros -- would leave something
    outside [0][0][:].  What they leave there is 32 times the line's spectrum, exactly, and the line's spectrum is the host build's."""
    exe, d = harness
    from pdb_eda_amd import ccp4, synthetic
    line = np.asarray(fc.grid_of("mixed")[0, 0, :], dtype=np.float32)
    grid = np.ascontiguousarray(np.broadcast_to(line, (4, 8, 30)), dtype=np.float32)
    spec = synthetic.MapSpec(ncrs=(30, 8, 4), spacing=0.5)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "rows", ctx=gpu_ctx)
    got = dm.fourier().values()
    lines, proc = fc.harness_lines(exe, d, [line.astype(np.complex128)], tag="one_line")
    assert proc.returncode == 0
    fwd = lines[0][0]
    assert same_bits(got[0, 0, :], 32.0 * fwd[:16])
    rest = got.copy()
    rest[0, 0, :] = 0.0
    assert not rest.any()


# ---- the round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.FORWARD + ("cut",))
def test_round_trip(gpu_ctx, name):
    """fourier().toMap(): |out - x| <= half a float32 ulp of x + 32 eps log2 N ||x||_2 per voxel, on the map's own header; twice the same bits."""
    dm, grid = device_map(name, gpu_ctx)
    spec = dm.fourier()
    out = spec.toMap()
    got = out.density
    assert list(out.header.ncrs) == list(dm.header.ncrs) and got.dtype == np.float32
    x = grid.astype(np.float64)
    bound = 0.5 * np.spacing(np.abs(grid)).astype(np.float64) + 32.0 * ck.EPS * np.log2(float(grid.size)) * float(np.sqrt((x * x).sum()))
    worst = float((np.abs(got.astype(np.float64) - x) / np.maximum(bound, 1e-300)).max()) if grid.size > 1 else 0.0
    print("%s: worst |out - x| / bound = %.3g; %d of %d voxels differ" % (name, worst, int((got != grid).sum()), grid.size))
    assert (np.abs(got.astype(np.float64) - x) <= bound).all()
    assert np.array_equal(spec.toMap().density.view(np.uint32), got.view(np.uint32))


# ---- scaled + toMap ------------------------------------------------------------------------------------------------------------------
def adjacent_or_equal(got, want):
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


@pytest.mark.parametrize("name", fc.FILTER_MAPS)
@pytest.mark.parametrize("which", ["blur", "sharpen", "cut3"])
def test_scaled_to_map_against_checker(gpu_ctx, name, which):
    """A B-factor blur, a sharpening and a soft 3 A cut: every voxel equal to the checker's or an adjacent float32, at most 1 in 10^4 unequal."""
    dm, grid = device_map(name, gpu_ctx)
    table, s2max, beyond = fc.filters(dm.header)[which]
    metric = fc.reciprocalMetric(dm.header)
    want = wanted(("scaled", name, which), lambda: ck.inverse(ck.scaled(ck.forward(grid), grid.shape, metric, table, s2max, beyond), grid.shape))
    got = dm.fourierFiltered(table, s2max, beyond).density
    unequal = int((got != want).sum())
    print("%s / %s: %d of %d voxels unequal" % (name, which, unequal, got.size))
    assert adjacent_or_equal(got, want).all()
    assert unequal * 10000 <= got.size
    assert float(np.abs(got - grid).max()) > 1e-3          # (the filter did something)
    spec = dm.fourier()
    assert same_bits(spec.scaled(table, s2max, beyond).values(), dm.fourier().scale(table, s2max, beyond).values())
    scaled_want = ck.scaled(ck.forward(grid), grid.shape, metric, table, s2max, beyond)
    assert ck.rel_l2(spec.scaled(table, s2max, beyond).values(), scaled_want) <= ck.forward_bound(grid.shape) + 2.0 * ck.EPS


def test_methods_on_top_of_scaled(gpu_ctx):
    from pdb_eda_amd import ccp4
    dm, grid = device_map("mixed", gpu_ctx)
    metric = fc.reciprocalMetric(dm.header)
    for got, (table, s2max) in ((dm.resolutionCut(3.0, softness=0.2), (ccp4.resolutionTable(3.0, None, 0.2), ((1.0 + 0.1) / 3.0) ** 2 * (1.0 + 2.0 ** -20))),
                                (dm.sharpened(-8.0), (ccp4.bFactorTable(-8.0, ccp4.maxS2(dm.header)), ccp4.maxS2(dm.header)))):
        want = ck.inverse(ck.scaled(ck.forward(grid), grid.shape, metric, table, s2max, 0.0), grid.shape)
        assert adjacent_or_equal(got.density, want).all() and int((got.density != want).sum()) * 10000 <= want.size


# ---- shells --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.GEOMETRIES)
def test_shells_against_checker(gpu_ctx, name):
    """Counts exact, sums within 1e-12 relative (the cross terms relative to sqrt(Saa Sbb)); the counts add up to N minus what the edges drop;
    the same bits from two calls; the fsc of a map with itself is 1."""
    dm, grid = device_map(name, gpu_ctx)
    other, grid_b = second_map(name, gpu_ctx)
    metric, edges = fc.reciprocalMetric(dm.header), fc.edges_of(name)
    assert ck.edge_clearance(grid.shape, metric, edges) > 1e-9
    a, b = dm.fourier(), other.fourier()
    count_w, sums_w = wanted(("shells", name), lambda: ck.shells(ck.forward(grid), ck.forward(grid_b), grid.shape, metric, edges))
    table = a.shells(b, edges=edges)
    assert np.array_equal(table["n"], count_w)
    sums = table["sums"]
    cross = np.sqrt(sums_w[:, 0] * sums_w[:, 1])
    rel = [np.abs(sums[:, 0] - sums_w[:, 0]) / sums_w[:, 0], np.abs(sums[:, 1] - sums_w[:, 1]) / sums_w[:, 1], np.abs(sums[:, 2] - sums_w[:, 2]) / cross,
           np.abs(sums[:, 3] - sums_w[:, 3]) / cross]
    print("%s: worst relative deviation of a shell sum %.3g" % (name, max(float(r.max()) for r in rel)))
    assert all(float(r.max()) <= 1e-12 for r in rel)
    s2 = ck.s2_grid(grid.shape, metric, half=False)
    dropped = int(((s2 < edges[0]) | (s2 >= edges[-1])).sum())
    assert int(table["n"].sum()) == grid.size - dropped and dropped >= 1          # (F(000) is in no shell)
    again = a.shells(b, edges=edges)
    assert same_bits(again["sums"], sums) and np.array_equal(again["n"], table["n"])
    fsc_w, scale_w = ck.shell_table(count_w, sums_w)
    assert np.allclose(table["fsc"], fsc_w, rtol=0, atol=1e-11) and np.allclose(table["scale"], scale_w, rtol=1e-10, atol=0)
    alone = a.shells(None, edges=edges)
    assert np.array_equal(alone["n"], count_w) and same_bits(alone["sums"][:, 0], sums[:, 0]) and not alone["sums"][:, 1:].any()
    itself = a.shells(a, edges=edges)
    assert np.allclose(itself["fsc"], 1.0, rtol=0, atol=1e-12) and not itself["sums"][:, 3].any()
    assert np.array_equal(dm.shellStats(other, nShells=12)["n"], count_w)


def test_fsc_with_the_resolution_cut(gpu_ctx):
    """A spectrum against itself cut at 3 A: fsc 1 in the shells inside the cut, undefined (the cut spectrum is exactly 0) in the shells beyond it.
    Through maps (``resolutionCut`` rounds to float32, whose rounding noise is spread over all shells and not correlated with the map) 1 to within
    1e-6 inside, and within 6 / sqrt(n) of 0 beyond: the standard deviation of the correlation of n independent terms is 1 / sqrt(n)."""
    from pdb_eda_amd import ccp4
    dm, grid = device_map("mixed", gpu_ctx)
    edges = ccp4.shellEdges(dm.header, 16, dMin=2.0)          # (shells of equal volume up to 2 A: three lie inside the cut, nine beyond it)
    soft = 0.2
    table = ccp4.resolutionTable(3.0, None, soft)
    s2max = ((1.0 + 0.5 * soft) / 3.0) ** 2 * (1.0 + 2.0 ** -20)
    a = dm.fourier()
    t = a.shells(a.scaled(table, s2max, 0.0), edges=edges)
    inside, beyond = edges[1:] <= ((1.0 - 0.5 * soft) / 3.0) ** 2, edges[:-1] >= s2max
    assert inside.sum() >= 2 and beyond.sum() >= 2
    assert np.allclose(t["fsc"][inside], 1.0, rtol=0, atol=1e-12) and np.isnan(t["fsc"][beyond]).all()
    m = dm.fsc(dm.resolutionCut(3.0, softness=soft), nShells=16, dMin=2.0)
    print("fsc of the map with its 3 A cut:", np.array2string(m["fsc"], precision=4))
    assert np.allclose(m["fsc"][inside], 1.0, rtol=0, atol=1e-6)
    assert (np.isnan(m["fsc"][beyond]) | (np.abs(m["fsc"][beyond]) <= 6.0 / np.sqrt(m["n"][beyond]))).all()


# ---- single coefficients -------------------------------------------------------------------------------------------------------------
INDICES = [(0, 0, 0), (1, 2, 3), (15, 18, 35), (16, 0, 0), (29, 35, 69), (-1, -2, -3), (-16, 5, -40), (31, 36, 70), (300, -300, 1000), (14, -17, 34)]


@pytest.mark.parametrize("name", ["mixed", "r753"])
def test_values_in_both_halves(gpu_ctx, name):
    dm, grid = device_map(name, gpu_ctx)
    want = ck.values(wanted(("fftn", name), lambda: ck.full(grid)), INDICES)
    got = dm.fourier().at(INDICES)
    scale = float(np.abs(ck.full(grid)).max())
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= ck.forward_bound(grid.shape) * scale * np.sqrt(grid.size)
    assert len(dm.fourier().at(np.zeros((0, 3), dtype=np.int32))) == 0


@pytest.mark.parametrize("name", ["mixed", "hex", "perm"])
def test_structure_factors(gpu_ctx, name):
    """F(hkl) of a whole-cell map, Miller indices on the cell axes, against the plain sum over the voxels."""
    dm, grid = device_map(name, gpu_ctx)
    hkl = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, -3, 5), (-7, 4, -1), (15, 17, 3), (-15, -18, -35)]
    want = ck.structure_factors(dm.header, grid, hkl)
    got = dm.structureFactors(hkl)
    assert float(np.abs(got - want).max()) <= 1e-10 * float(np.abs(want).max())
    assert abs(got[0].imag) <= 1e-9 * abs(got[0].real) and got[0].real > 0


def test_structure_factors_carry_the_phase_of_crs_start(gpu_ctx):
    """The same density stored with another crsStart is the same crystal moved: |F| stays, the phase turns by 2 pi h . start / interval."""
    from pdb_eda_amd import ccp4, synthetic
    grid = fc.grid_of("mixed")
    spec = synthetic.MapSpec(ncrs=(30, 36, 70), crs_start=(4, -5, 9), spacing=0.5)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "moved", ctx=gpu_ctx)
    hkl = [(1, 0, 0), (2, -3, 5), (-7, 4, -1)]
    want = ck.structure_factors(dm.header, grid, hkl)
    got = dm.structureFactors(hkl)
    assert float(np.abs(got - want).max()) <= 1e-10 * float(np.abs(want).max())
    cut, _ = device_map("cut", gpu_ctx)
    with pytest.raises(ValueError):
        cut.structureFactors(hkl)


def test_fourier_box_embeds_in_zeros(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic
    grid = np.ascontiguousarray(fc.grid_of("mixed")[:13, :11, :17])
    spec = synthetic.MapSpec(ncrs=(17, 11, 13), interval=(120, 120, 120), crs_start=(3, -2, 5), spacing=0.5)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "small", ctx=gpu_ctx)
    with pytest.raises(Exception):
        dm.fourier()
    box = dm.fourierBox(1.0)
    assert list(box.header.ncrs) == [21, 15, 18] and list(box.header.crsStart) == [1, -4, 3]
    want = np.zeros((18, 15, 21), dtype=np.float32)
    want[2:15, 2:13, 2:19] = grid
    assert np.array_equal(box.density, want)
    assert ck.rel_l2(box.fourier().values(), ck.forward(want)) <= ck.forward_bound(want.shape)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic, _native
    lib = gpu_ctx._lib
    for ncrs, axis, nxt in (((11, 4, 4), "c", "12"), ((4, 13, 4), "r", "14"), ((2, 2, 2048), "s", "no next")):
        grid = np.ones((ncrs[2], ncrs[1], ncrs[0]), dtype=np.float32)
        dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(synthetic.MapSpec(ncrs=ncrs, spacing=0.5), grid)), "bad", ctx=gpu_ctx)
        out = ctypes.c_void_p(0x5A5A)
        rc = lib.pdbeda_map_fft(dm._map._h, ctypes.byref(out))
        msg = lib.pdbeda_last_error(gpu_ctx._h).decode()
        assert rc == _native.PDBEDA_ERR_ARGUMENT and out.value == 0x5A5A and ("axis " + axis) in msg and nxt in msg, msg
        with pytest.raises(_native.PdbedaError):
            dm.fourier()
    dm, grid = device_map("mixed", gpu_ctx)
    other, _ = device_map("r753", gpu_ctx)
    spec = dm.fourier()
    before = spec.values()
    out = ctypes.c_void_p(0x5A5A)
    assert lib.pdbeda_spectrum_inverse(spec._spec._h, other._map._h, ctypes.byref(out)) == _native.PDBEDA_ERR_ARGUMENT and out.value == 0x5A5A
    assert lib.pdbeda_map_fft(None, ctypes.byref(out)) == _native.PDBEDA_ERR_ARGUMENT and lib.pdbeda_map_fft(dm._map._h, None) == _native.PDBEDA_ERR_ARGUMENT
    metric, edges = fc.reciprocalMetric(dm.header), fc.edges_of("mixed")
    bad_metric = metric.copy()
    bad_metric[4] = np.nan
    for call in (lambda: spec.shells(None, edges=edges[::-1]), lambda: spec.shells(None, edges=[0.1, 0.1, 0.2]), lambda: spec.shells(None, edges=[0.1]),
                 lambda: spec.shells(None, edges=[0.1, np.inf]), lambda: spec.shells(None, edges=np.linspace(0.01, 1.0, 258)),
                 lambda: spec.shells(other.fourier(), edges=edges), lambda: spec.scale([1.0], 1.0), lambda: spec.scale(np.ones(4097), 1.0),
                 lambda: spec.scale([1.0, np.nan], 1.0), lambda: spec.scale([1.0, 0.5], 0.0), lambda: spec.scale([1.0, 0.5], np.inf),
                 lambda: spec.scale([1.0, 0.5], 1.0, beyond=np.nan), lambda: spec._spec.scale(bad_metric, np.ones(2), 1.0),
                 lambda: spec._spec.shells(None, bad_metric, edges)):
        with pytest.raises(_native.PdbedaError):
            call()
    count = np.full(12, -7, dtype=np.int64)
    sums = np.full((12, 4), -7.0)
    rc = lib.pdbeda_spectrum_shells(spec._spec._h, None, metric.ctypes.data_as(ctypes.c_void_p), edges[::-1].copy().ctypes.data_as(ctypes.c_void_p), 12,
                                    count.ctypes.data_as(ctypes.c_void_p), sums.ctypes.data_as(ctypes.c_void_p))
    assert rc == _native.PDBEDA_ERR_ARGUMENT and (count == -7).all() and (sums == -7.0).all()
    assert same_bits(spec.values(), before)          # (no refused scale touched the spectrum)
    assert ck.rel_l2(dm.fourier().values(), ck.forward(grid)) <= ck.forward_bound(grid.shape)          # (the context still works)


# ---- the analysis level --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analyzer(gpu_ctx):
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    z, spec, st, pdb, params = load_analysis_case("orth")
    densityAnalysis.setGlobals(params)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), "orth", ctx=gpu_ctx)
    diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), "orth", ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(dens, diff)
    st.header = {"resolution": 2.0}
    return densityAnalysis.DensityAnalysis("orth", dens, diff, st, pdb)


def test_model_shell_table_and_fsc_resolution(analyzer):
    """The entry's cell is sampled 72 x 64 x 68: 68 is not plannable, so the map goes to 72 x 64 x 70 first.  The table and the crossing against the
    same quantities from the downloaded maps."""
    from pdb_eda_amd import ccp4, singleStructure
    observed, model = analyzer._fourierMaps()
    assert list(observed.header.ncrs) == [72, 64, 70] and list(model.header.ncrs) == [72, 64, 70]
    a, b = observed.density, model.density
    assert float(b.max()) > 0.1
    metric, edges = ccp4.reciprocalMetric(observed.header), ccp4.shellEdges(observed.header, 20)
    assert ck.edge_clearance(a.shape, metric, edges) > 1e-9
    count_w, sums_w = ck.shells(ck.forward(a), ck.forward(b), a.shape, metric, edges)
    fsc_w, scale_w = ck.shell_table(count_w, sums_w)
    table = analyzer.modelShellTable(20)
    print("map-model fsc per shell:", np.array2string(table["fsc"], precision=3))
    assert np.array_equal(table["n"], count_w)
    assert np.allclose(table["fsc"], fsc_w, rtol=0, atol=1e-10) and np.allclose(table["scale"], scale_w, rtol=1e-9, atol=0)
    assert float(np.nanmax(table["fsc"])) > 0.5          # (the model explains its own map at low resolution)
    s = 0.5 * (np.sqrt(edges[:-1]) + np.sqrt(edges[1:]))
    for threshold in (0.5, 0.143, 2.0):
        want = ck.crossing(s, fsc_w, threshold)
        got = analyzer.fscResolution(threshold)
        assert (got is None) == (want is None)
        if want is not None:
            assert abs(got - 1.0 / want) <= 1e-8 * got
    summary = analyzer.fourierSummary()
    assert summary["grid_s"] == 70 and summary["fsc_05_resolution"] == analyzer.fscResolution(0.5)
    header, rows = singleStructure.rows(analyzer, "fourier", "shell")
    assert header == analyzer.fourierShellHeader and len(rows) == 20 and rows[3][3] == int(count_w[3])
    header, rows = singleStructure.rows(analyzer, "fourier", "summary")
    assert len(rows) == 1 and len(rows[0]) == len(header)
    cut = analyzer.resolutionCutDensityObj(3.0)
    assert list(cut.header.ncrs) == [72, 64, 70] and np.isfinite(cut.density).all()
    assert list(analyzer.sharpenedDensityObj(-10.0).header.ncrs) == [72, 64, 70]
