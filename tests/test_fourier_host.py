"""Reciprocal space without a GPU.  pdb_eda_amd/csrc/pdbeda_fourier_line.h -- the planner, the twiddle table and the line transform the kernels run --
through tests/fourier_harness.cpp, built with the host compiler under AddressSanitizer + UBSan (nothing recovered, nothing preloaded): every
plannable length from 1 to 1024 in both directions against numpy.fft, within 16 * 2^-53 * max(1, log2 n) relative L2 (the classical bound is about
7 eps per radix-2 stage and numpy's own result carries as much; 16 covers the two -- a plain matrix DFT stays at 9 to 11 in these units).  Then the
host-side Python of ccp4.py (metric, shells, tables, sizes), tests/fourier_checker.py against itself and scipy, and the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import fourier_cases as fc
import fourier_checker as ck

from pdb_eda_amd import ccp4

PLANNABLE = [n for n in range(1, fc.MAX_AXIS + 1) if ccp4.isFourierSize(n)]


def seeded_line(n):
    rng = np.random.default_rng(9000 + n)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) + (0.75 - 0.25j)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("fourier_host")
    exe = fc.build_harness(d, sanitize=True)
    lines = [seeded_line(n) for n in PLANNABLE]
    out, proc = fc.harness_lines(exe, d, lines)
    plan = subprocess.run([exe, "plan", "-2", "2100"], capture_output=True, text=True, timeout=120)
    return {"exe": exe, "dir": d, "lines": lines, "out": out, "proc": proc, "plan": plan}


def test_the_harness_ends_clean_under_the_sanitizers(run):
    assert run["proc"].returncode == 0 and run["proc"].stderr == "", run["proc"].stderr[-4000:]
    assert run["plan"].returncode == 0 and run["plan"].stderr == "", run["plan"].stderr[-4000:]
    assert len(run["out"]) == len(PLANNABLE)


def test_the_plan_is_a_function_of_n_alone(run):
    """Plannable iff 2^a 3^b 5^c 7^d within 1 .. 1024; the radices multiply to n and come as 4 (a / 2 times), 2 (if a is odd), 3, 5, 7; the
    next plannable length is ccp4.fourierSize's."""
    rows = [line.split() for line in run["plan"].stdout.splitlines()]
    assert [int(r[0]) for r in rows] == list(range(-2, 2101))
    most = 0
    for r in rows:
        n, ok, nxt = int(r[0]), int(r[1]), int(r[2])
        assert ok == (1 if ccp4.isFourierSize(n) else 0), n
        assert nxt == (ccp4.fourierSize(n) if n <= fc.MAX_AXIS else 0), n
        if ok:
            radices = [int(v) for v in r[4:]]
            a = 0
            while n % (2 ** (a + 1)) == 0:
                a += 1
            rest, want = n // 2 ** a, [4] * (a // 2) + [2] * (a % 2)
            for p in (3, 5, 7):
                while rest % p == 0:
                    want.append(p)
                    rest //= p
            assert radices == want and int(r[3]) == len(want), n
            most = max(most, len(want))
    assert most == 6 and len(PLANNABLE) == sum(int(r[1]) for r in rows)


@pytest.mark.parametrize("inverse", [0, 1])
def test_every_plannable_line_against_numpy(run, inverse):
    worst = (0.0, 0)
    for x, got in zip(run["lines"], run["out"]):
        n = len(x)
        want = np.fft.ifft(x) * n if inverse else np.fft.fft(x)
        units = ck.rel_l2(got[inverse], want) / (ck.EPS * max(1.0, float(np.log2(n))))
        worst = max(worst, (units, n))
        assert units <= 16.0, (n, units)
    print("%s: worst relative L2 error %.2f eps max(1, log2 n), at n = %d" % ("inverse" if inverse else "forward", worst[0], worst[1]))


def reference_twiddles(n):
    """exp(-2 pi i k / n), k = 0 .. n - 1, in extended precision (re, im): the angle reduced to an octant in integers, so that the argument of sin / cos
    is at most pi / 4 and exact but for one rounding; numpy's long double (64 bits of mantissa here) carries 11 bits more than the table."""
    ld = np.longdouble
    half_pi = ld(2) * np.arctan(ld(1))
    q, r = np.divmod(4 * np.arange(n, dtype=np.int64), n)
    low = 2 * r <= n
    phi = half_pi * np.where(low, r, n - r).astype(ld) / ld(n)
    c, s = np.where(low, np.cos(phi), np.sin(phi)), np.where(low, np.sin(phi), np.cos(phi))
    c, s = np.where(r == 0, ld(1), c), np.where(r == 0, ld(0), s)
    co = np.choose(q % 4, [c, -s, -c, s])
    si = np.choose(q % 4, [s, c, -s, -c])
    return co, -si


@pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="numpy's long double is no wider than a double here")
def test_the_twiddle_table_is_within_one_ulp(run):
    for x, got in zip(run["lines"], run["out"]):
        n, w = len(x), got[2]
        for have, want in zip((w.real, w.imag), reference_twiddles(n)):
            assert (np.abs(have.astype(np.longdouble) - want) <= np.spacing(np.abs(want).astype(np.float64))).all(), n
            zero = want == 0
            assert (have[zero] == 0.0).all() and not np.signbit(have[zero]).any(), n


def test_the_exact_entries_are_exact(run):
    for x, got in zip(run["lines"], run["out"]):
        n, w = len(x), got[2]
        assert w[0] == 1.0
        if n % 2 == 0:
            assert w[n // 2] == -1.0
        if n % 4 == 0:
            assert w[n // 4] == -1j and w[3 * n // 4] == 1j
        if n % 8 == 0:
            assert w[n // 8].real == -w[n // 8].imag
        assert not np.signbit(w.real[w.real == 0]).any() and not np.signbit(w.imag[w.imag == 0]).any()
        for k in range(1, n):      # the symmetries of the circle
            assert w[n - k] == np.conj(w[k]), (n, k)


def test_lengths_that_are_not_plannable_are_refused(run):
    for n in (11, 13, 17, 1025, 2048):
        out, proc = fc.harness_lines(run["exe"], run["dir"], [np.ones(n, dtype=np.complex128)], tag="refused")
        assert proc.returncode == 3 and out == []
    src, dst = os.path.join(str(run["dir"]), "bad.in"), os.path.join(str(run["dir"]), "bad.out")
    with open(src, "wb") as f:
        f.write(np.array([4, 11, 4], dtype=np.int32).tobytes() + np.zeros(176, dtype=np.float32).tobytes())
    assert subprocess.run([run["exe"], "volume", src, dst], capture_output=True, timeout=60).returncode == 3
    assert not ccp4.isFourierSize(0) and not ccp4.isFourierSize(11) and not ccp4.isFourierSize(2048) and ccp4.isFourierSize(1024)
    with pytest.raises(ValueError):
        ccp4.fourierSize(1025)


@pytest.mark.parametrize("name", ["one", "r235", "r753", "p4", "mixed", "longc", "longr", "longs", "tile_past", "cols_past"])
def test_the_harness_volume_against_the_checker(run, name):
    """The 3-D half spectrum the GPU test compares with to the bit is itself within the forward bound of numpy's."""
    grid = fc.grid_of(name)
    got = fc.harness_volume(run["exe"], run["dir"], grid, name)
    assert ck.rel_l2(got, ck.forward(grid)) <= ck.forward_bound(grid.shape)


# ---- the host side of ccp4.py --------------------------------------------------------------------------------------------------------
def brute_s2(header, h):
    """1 / d^2 of frequency numbers h (crs order) of the stored box from deOrthoMat: the box's frequency h along crs axis k is the cell's index
    h * crsInterval / ncrs along the xyz axis that crs axis runs along, and s = deOrthoMat^T hkl."""
    hkl = np.zeros(3)
    for k in range(3):
        hkl[header.map2crs[k]] = h[k] * float(header.crsInterval[k]) / float(header.ncrs[k])
    s = np.asarray(header.deOrthoMat, dtype=np.float64).T.dot(hkl)
    return float(s.dot(s))


@pytest.mark.parametrize("name", ["mixed", "hex", "perm", "cut"])
def test_reciprocal_metric_against_brute_force(name):
    header = fc.header_of(name)
    m = ccp4.reciprocalMetric(header)
    rng = np.random.default_rng(5)
    for h in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 2)] + [tuple(int(v) for v in rng.integers(-15, 16, 3)) for _ in range(40)]:
        got = float((m[0] * h[0] * h[0] + m[1] * h[1] * h[1] + m[2] * h[2] * h[2]) + 2.0 * (m[3] * h[0] * h[1] + m[4] * h[0] * h[2] + m[5] * h[1] * h[2]))
        want = brute_s2(header, h)
        assert abs(got - want) <= 1e-12 * max(want, 1e-30), (name, h)
    if name == "mixed":      # 0.5 A steps: the (1, 0, 0) plane of a 15 A edge
        assert abs(m[0] - 1.0 / 15.0 ** 2) < 1e-12 and abs(m[3]) < 1e-18
    if name == "hex":        # gamma = 120: a* . b* > 0
        assert m[3] > 0 and abs(m[4]) < 1e-18 and abs(m[5]) < 1e-18


def test_s2_grid_uses_the_frequency_numbers():
    assert ck.freq(6).tolist() == [0, 1, 2, 3, -2, -1] and ck.freq(5).tolist() == [0, 1, 2, -2, -1] and ck.freq(1).tolist() == [0]
    header = fc.header_of("hex")
    m = ccp4.reciprocalMetric(header)
    s2 = ck.s2_grid(fc.shape_of("hex"), m, half=False)
    for s, r, c in [(0, 0, 0), (3, 5, 7), (69, 35, 29), (35, 18, 15), (40, 2, 20)]:
        h = (int(ck.freq(30)[c]), int(ck.freq(36)[r]), int(ck.freq(70)[s]))
        assert abs(s2[s, r, c] - brute_s2(header, h)) <= 1e-12 * max(s2[s, r, c], 1e-30)


def test_shell_edges():
    header = fc.header_of("mixed")
    e = ccp4.shellEdges(header, 20)
    assert len(e) == 21 and (np.diff(e) > 0).all() and e[0] > 0
    assert np.allclose(np.diff(e ** 1.5), (e[-1] ** 1.5 - e[0] ** 1.5) / 20, rtol=1e-9)          # equal steps of s^3
    assert 1.0 < e[-1] <= 1.0 * (1.0 + 2.0 ** -18)          # the Nyquist limit of a 0.5 A grid is 1 A, and the edge lies just above it
    assert e[0] < ccp4.reciprocalMetric(header)[2]          # below the first reflection of the longest axis
    e = ccp4.shellEdges(header, 5, dMin=2.0, dMax=10.0)
    assert abs(e[0] - 0.01) < 1e-15 and abs(e[-1] - 0.25) < 1e-15
    coarse = fc.header_of("hex")      # 15 / 30, 18 / 36 and 35 / 70 A steps along a, b, c with gamma = 120: a* and b* are longer by 1 / sin 120
    assert abs(np.sqrt(ccp4.shellEdges(coarse, 4)[-1]) - 1.0) < 1e-5
    for bad in (lambda: ccp4.shellEdges(header, 0), lambda: ccp4.shellEdges(header, 257), lambda: ccp4.shellEdges(header, 4, dMin=3.0, dMax=2.0)):
        with pytest.raises(ValueError):
            bad()


def test_tables():
    t = ccp4.bFactorTable(20.0, 0.5, 11)
    assert len(t) == 11 and t[0] == 1.0 and abs(t[-1] - np.exp(-2.5)) < 1e-15 and (np.diff(t) < 0).all()
    assert (np.diff(ccp4.bFactorTable(-20.0, 0.5, 11)) > 0).all()
    g = ccp4.resolutionTable(3.0, None, 0.2, n=2049)
    s = np.sqrt(np.linspace(0.0, ((1.1) / 3.0) ** 2 * (1.0 + 2.0 ** -20), 2049))
    assert (g[s <= 0.3] == 1.0).all() and g[-1] < 1e-9 and (np.diff(g) <= 0).all() and g.min() >= 0.0
    assert abs(np.interp(1.0 / 3.0, s, g) - 0.5) < 1e-3
    step = ccp4.resolutionTable(3.0, None, 0.0, s2Max=0.25, n=1001)
    assert set(np.unique(step)) == {0.0, 1.0}
    band = ccp4.resolutionTable(3.0, 10.0, 0.1, n=4096)
    assert band[0] == 0.0 and band.max() == 1.0 and band[-1] < 1e-9
    with pytest.raises(ValueError):
        ccp4.resolutionTable()
    assert len(ccp4.resolutionTable(3.0)) <= ccp4.SPECTRUM_MAX_TABLE


def test_fourier_sizes_and_header():
    assert [ccp4.fourierSize(n) for n in (0, 1, 11, 13, 17, 68, 97, 1000, 1023)] == [1, 1, 12, 14, 18, 70, 98, 1000, 1024]
    spec = fc.synthetic.MapSpec(ncrs=(20, 17, 9), interval=(68, 44, 26), crs_start=(3, 4, 5), axis_order=(2, 1, 3), cell=(34.0, 22.0, 13.0))
    import io
    header = ccp4.read_grid(io.BytesIO(fc.synthetic.ccp4_bytes(spec, np.zeros((9, 17, 20), dtype=np.float32))))[0]
    f = ccp4.fourierHeader(header)
    assert list(f.xyzInterval) == [70, 45, 27] and list(f.ncrs) == [45, 70, 27] and list(f.crsStart) == [0, 0, 0] and list(f.ncrs) == list(f.crsInterval)
    assert np.allclose(f.orthoMat, header.orthoMat) and (f.col2xyz, f.row2xyz, f.sec2xyz) == (2, 1, 3)
    whole = fc.header_of("mixed")
    assert list(ccp4.fourierHeader(whole).ncrs) == list(ccp4.cellHeader(whole).ncrs)
    assert ccp4.maxS2(whole) >= float(ck.s2_grid(fc.shape_of("mixed"), ccp4.reciprocalMetric(whole)).max())


# ---- the checker against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.GEOMETRIES + ("r753", "p4"))
def test_shell_sums_from_the_half_equal_those_from_the_full_spectrum(name):
    grid, other = fc.grid_of(name), fc.grid_of(name, seed=1, offset=-0.5)
    metric = ccp4.reciprocalMetric(fc.header_of(name))
    edges = fc.edges_of(name, 12 if name in fc.GEOMETRIES else 3)
    assert ck.edge_clearance(grid.shape, metric, edges) > 1e-9          # no s^2 sits on an edge: the counts are a fair exact comparison
    count_h, sums_h = ck.shells(ck.forward(grid), ck.forward(other), grid.shape, metric, edges)
    count_f, sums_f = ck.shells_full(ck.full(grid), ck.full(other), grid.shape, metric, edges)
    assert np.array_equal(count_h, count_f) and count_h.sum() > 0
    cross = np.sqrt(sums_f[:, 0] * sums_f[:, 1])
    assert np.allclose(sums_h[:, :2], sums_f[:, :2], rtol=1e-12, atol=0)
    assert (np.abs(sums_h[:, 2] - sums_f[:, 2]) <= 1e-12 * cross).all()
    # Im(A conj B) of a coefficient and of its Hermitian mirror cancel: over the FULL spectrum of two real maps the sum vanishes, and the contract's
    # fourth sum is that of the STORED half under the weights 1 and 2 -- a number that tells a shift between the maps, not zero
    # (on a skewed cell a coefficient of a Nyquist plane, h = + n / 2, and its mirror, which is stored at the same index, differ in s^2: only cells
    #  without cross terms are asked to cancel shell by shell)
    assert float(np.abs(sums_h[:, 3]).max()) > 0 and (np.any(metric[3:] != 0) or (np.abs(sums_f[:, 3]) <= 1e-12 * cross).all())
    assert ck.shell_of(np.array([edges[0], edges[1], np.nextafter(edges[1], 0), edges[-1], 0.0]), edges).tolist() == [0, 1, 0, -1, -1]


def test_the_gain_rule():
    table = np.array([1.0, 0.5, 0.25, 4.0])
    s2 = np.array([0.0, 0.5, 1.0, 1.5, 2.75, 3.0, np.nextafter(3.0, 4.0), 7.0])
    assert ck.gain(s2, table, 3.0, -9.0).tolist() == [1.0, 0.75, 0.5, 0.375, 0.25 + 0.75 * 3.75, 4.0, -9.0, -9.0]


@pytest.mark.parametrize("name", fc.FILTER_MAPS)
def test_the_reference_alone_meets_the_cap_on_unequal_voxels(name):
    """The GPU test allows 1 voxel in 10^4 to differ from numpy's by one float32 step.  Two references -- numpy.fft and scipy.fft -- against each
    other stay inside the same cap, so it holds for the reference alone."""
    import scipy.fft as scipy_fft
    grid = fc.grid_of(name)
    header = fc.header_of(name)
    metric = ccp4.reciprocalMetric(header)
    for which, (table, s2max, beyond) in fc.filters(header).items():
        g = ck.gain(ck.s2_grid(grid.shape, metric), table, s2max, beyond)
        a = ck.inverse(ck.scaled(ck.forward(grid), grid.shape, metric, table, s2max, beyond), grid.shape)
        f = scipy_fft.rfftn(grid.astype(np.float64))
        b = scipy_fft.irfftn(f.real * g + 1j * (f.imag * g), s=grid.shape).astype(np.float32)
        unequal = int((a != b).sum())
        print("%s / %s: numpy.fft and scipy.fft differ in %d of %d voxels" % (name, which, unequal, a.size))
        assert unequal * 10000 <= a.size
        assert ((a == b) | (a == np.nextafter(b, np.float32(np.inf))) | (a == np.nextafter(b, np.float32(-np.inf)))).all()
        assert float(np.abs(a - grid).max()) > 1e-3


def test_structure_factor_restatement():
    """F(000) is the cell's content, and a shifted crsStart turns the phase."""
    header, grid = fc.header_of("hex"), fc.grid_of("hex")
    f = ck.structure_factors(header, grid, [(0, 0, 0), (1, 2, -3)])
    volume = header.unitVolume * grid.size
    assert abs(f[0] - volume * float(grid.astype(np.float64).mean())) <= 1e-9 * abs(f[0])
    assert abs(f[1]) < abs(f[0])


def test_crossing():
    s = np.array([0.1, 0.2, 0.3, 0.4])
    assert abs(ck.crossing(s, np.array([0.9, 0.7, 0.3, 0.6]), 0.5) - 0.25) < 1e-15
    assert ck.crossing(s, np.array([0.9, 0.8, 0.7, 0.6]), 0.5) is None and ck.crossing(s, np.array([0.9, np.nan, 0.3, 0.2]), 0.5) is None


# ---- the binding ---------------------------------------------------------------------------------------------------------------------
def test_the_binding_and_the_modes():
    from pdb_eda_amd import _native, densityAnalysis, singleStructure
    names = ("pdbeda_map_fft", "pdbeda_spectrum_inverse", "pdbeda_spectrum_shape", "pdbeda_spectrum_download", "pdbeda_spectrum_free", "pdbeda_spectrum_values",
             "pdbeda_spectrum_scale", "pdbeda_spectrum_shells")
    text = open(os.path.join(fc.ROOT, "include", "pdbeda.h")).read()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, text)
    assert len(_native.EXPORTED_SYMBOLS) >= 80
    for define, value in (("PDBEDA_FFT_MAX_AXIS", _native.FFT_MAX_AXIS), ("PDBEDA_SPECTRUM_MAX_TABLE", _native.SPECTRUM_MAX_TABLE), ("PDBEDA_SPECTRUM_MAX_SHELLS", _native.SPECTRUM_MAX_SHELLS)):
        assert "#define %s %d" % (define, value) in text
    assert "fourier" in singleStructure.MODES and all(("fourier", level) in singleStructure.TABLES for level in ("shell", "summary"))
    for name in ("modelShellTable", "fscResolution", "resolutionCutDensityObj", "sharpenedDensityObj", "fourierSummary"):
        assert callable(getattr(densityAnalysis.DensityAnalysis, name))
    for name in ("fourier", "fourierFiltered", "resolutionCut", "sharpened", "shellStats", "fsc", "structureFactors", "fourierBox"):
        assert callable(getattr(ccp4.DensityMatrix, name))
    for name in ("shape", "values", "at", "scaled", "toMap", "shells"):
        assert hasattr(ccp4.DensitySpectrum, name)
