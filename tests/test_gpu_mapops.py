"""The small whole-map kernels at their edges (inputs: tests/mapops_cases.py, all of them checked on the CPU by
tests/test_mapops_host.py; yardstick: tests/mapops_checker.py, numpy in fp64):

k_map_combine       pdbeda_map_combine + pdbeda_map_download == the checker to the bit, at 4.25 M voxels (second trip of the float4
                    loop, two tail lanes), at n = 1..7 and 1 023 and on the value edges (subnormals in and out, overflow to inf);
k_abs_select_hist   every histogram of pdbeda_abs_select_hist == the checker's, at every shift, with and without a prefix, on the big map
                    (five trips), the tails, boxes that repeat along c, r, s and under a permuted axis order, voxels on the cuts, +-0,
                    NaN, inf, subnormals, long runs of equal keys, and keys with busy low digits; DeviceMap.abs_order_statistics and
                    DensityAnalysis.medianAbsFoFc on top of them;
k_reduce_partials   pdbeda_sum_of_abs within d * 2^-53 * sum |x| of math.fsum, d counted from the kernels (sum_chain_depth);
k_byteswap32        a big-endian file arrives as its grid, to the bit, with the statistics of that grid.

A NaN that an operation makes has no bits to compare (mapops_checker.same_bits); everything else is compared with ==."""
import ctypes as C
import io
import math
import time

import numpy as np
import pytest

import mapops_cases as cases
import mapops_checker as checker

pytestmark = pytest.mark.gpu

F4, F8 = np.float32, np.float64
SMALL_NAMES = ["tail_%d" % n for n in (1, 2, 3, 4, 5, 7, 1023)] + list(cases.GEOMETRY) + ["edges", "ties_even", "ties_odd", "low_digits"]
TAIL_NAMES = SMALL_NAMES[:7]


class Borrowed(object):
    """A DeviceMap on a buffer that the library does not own (pdbeda_map_from_device).  The buffer comes from the HIP runtime that the
    library itself is linked against: a symbol looked up through the library's handle is found in its dependencies."""

    def __init__(self, ctx, grid, geometry):
        from pdb_eda_amd import _native
        self.hip = _native.lib()
        grid = np.ascontiguousarray(grid, dtype=F4)
        self.ptr = C.c_void_p()
        malloc, copy = self.hip.hipMalloc, self.hip.hipMemcpy
        malloc.argtypes, copy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert malloc(C.byref(self.ptr), grid.nbytes) == 0
        assert copy(self.ptr, grid.ctypes.data_as(C.c_void_p), grid.nbytes, 1) == 0          # hipMemcpyHostToDevice, done when it returns
        self.ctx = ctx
        self.map = _native.DeviceMap(ctx, grid, geometry, device_ptr=self.ptr.value)

    def free(self):
        self.map.free()
        self.ctx.synchronize()
        release = self.hip.hipFree
        release.argtypes = [C.c_void_p]
        assert release(self.ptr) == 0


class World(object):
    def __init__(self, ctx):
        t0 = time.perf_counter()
        self.ctx = ctx
        self.case = {c.name: c for c in cases.small_cases()}
        self.case["big"] = cases.big()
        self.maps = {}
        print("mapops: %d cases made in %.2f s on the host" % (len(self.case), time.perf_counter() - t0))

    def device(self, grid, c, ctx=None):
        from pdb_eda_amd import _native
        return _native.DeviceMap(ctx or self.ctx, grid, c.header.geometry())

    def pair(self, name):
        if name not in self.maps:
            c = self.case[name]
            self.maps[name] = (self.device(c.a, c), self.device(c.b, c))
        return self.maps[name]

    def close(self):
        for pair in self.maps.values():
            for m in pair:
                m.free()


@pytest.fixture(scope="module")
def w(gpu_ctx):
    world = World(gpu_ctx)
    yield world
    world.close()


@pytest.fixture(scope="module")
def prof_ctx():
    from pdb_eda_amd import _native
    ctx = _native.Context(0)
    yield ctx
    ctx.close()


def big_endian_file(c, grid, path, big_endian=True):
    from pdb_eda_amd import synthetic
    with np.errstate(invalid="ignore"):                      # (the header's statistics of a grid that holds infinities)
        path.write_bytes(synthetic.ccp4_bytes(c.spec, grid, big_endian=big_endian))
    return str(path)


# ---- combine ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big"] + TAIL_NAMES + ["edges"])
def test_combine_gives_numpy_bits(w, name):
    from pdb_eda_amd import _native
    c = w.case[name]
    da, db = w.pair(name)
    for alpha in cases.ALPHAS:
        out = _native.DeviceMap.combine(da, db, alpha)
        got = out.download()
        out.free()
        want = checker.combine(c.a, c.b, alpha)
        assert got.shape == c.a.shape and checker.same_bits(got, want), (alpha, np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))[:8])
    assert np.array_equal(da.download().view(np.uint32), c.a.view(np.uint32))            # the operands are as they were
    assert np.array_equal(db.download().view(np.uint32), c.b.view(np.uint32))


@pytest.mark.parametrize("name", ["tail_1023", "edges"])
def test_combine_with_itself_and_with_a_borrowed_buffer(w, name):
    from pdb_eda_amd import _native
    c = w.case[name]
    da, db = w.pair(name)
    twin = w.device(c.a, c)
    lent = Borrowed(w.ctx, c.b, c.header.geometry())
    try:
        for alpha in cases.ALPHAS:
            one, two, three, four = (_native.DeviceMap.combine(x, y, alpha) for x, y in ((da, da), (da, twin), (da, lent.map), (lent.map, da)))
            got = [m.download() for m in (one, two, three, four)]
            for m in (one, two, three, four):
                m.free()
            assert checker.same_bits(got[0], checker.combine(c.a, c.a, alpha)) and checker.same_bits(got[1], got[0])
            assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))                      # (the NaNs too: the same device made both)
            assert checker.same_bits(got[2], checker.combine(c.a, c.b, alpha)) and checker.same_bits(got[3], checker.combine(c.b, c.a, alpha))
    finally:
        twin.free()
        lent.free()


def test_combined_map_is_labelled_like_an_uploaded_one(w):
    """A derived map gets a quantum of its own for the blob sums: the full-map labelling of a - 2 b at 1.5 sigma gives, row for row
    and bit for bit, what the same values uploaded from the host give."""
    from pdb_eda_amd import _native
    c = w.case["low_digits"]
    da, db = w.pair("low_digits")
    made = _native.DeviceMap.combine(da, db, -2.0)
    sent = w.device(checker.combine(c.a, c.b, -2.0), c)
    mean, std = sent.stats()
    assert made.stats() == (mean, std)
    cut = mean + 1.5 * std
    a, b = made.full_blobs(cut), sent.full_blobs(cut)
    sa, sb = a.stats(), b.stats()
    assert len(a) == len(b) > 20 and sorted(sa) == sorted(sb)
    for k in sa:
        assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), k
    for m in (a, b, made, sent):
        m.free()


def test_combine_refusals_leave_the_context_working(w):
    from pdb_eda_amd import _native
    c, other_shape = w.case["tail_1023"], w.case["tail_7"]
    da, db = w.pair("tail_1023")
    elsewhere = _native.Context(0)
    foreign = w.device(c.b, c, ctx=elsewhere)
    with pytest.raises(_native.PdbedaError):
        _native.DeviceMap.combine(da, foreign, 1.0)
    with pytest.raises(_native.PdbedaError):
        _native.DeviceMap.combine(da, w.pair("tail_7")[0], 1.0)
    assert other_shape.n != c.n
    out = _native.DeviceMap.combine(da, db, 1.0)
    assert checker.same_bits(out.download(), checker.combine(c.a, c.b, 1.0))
    back = _native.DeviceMap.combine(foreign, foreign, 1.0)                                   # the other context works too
    assert checker.same_bits(back.download(), checker.combine(c.b, c.b, 1.0))
    for m in (out, back, foreign):
        m.free()
    elsewhere.close()


# ---- select through the C ABI ----------------------------------------------------------------------------------------------------
def hist_call(w, a, b, alpha, cut_a, cut_b, which, shift, prefix, mask):
    out = np.full(65536, 0xdeadbeef, dtype=np.uint32)
    rc = w.ctx._lib.pdbeda_abs_select_hist(a._h, b._h if b is not None else None, alpha, cut_a, cut_b, which, shift, prefix, mask, out.ctypes.data_as(C.c_void_p))
    return rc, out.astype(np.int64)


def walk_prefixes(keys, rank):
    """(shift, prefix, mask) of every pass of the digit walk to ``rank``."""
    from pdb_eda_amd import _native
    seen = []

    def digit(shift, prefix, mask):
        seen.append((shift, prefix, mask))
        return checker.select_hist(keys, shift, prefix, mask)
    _native.radix_select(digit, 64 if keys.dtype == np.uint64 else 32, [rank])
    return seen


@pytest.mark.parametrize("name", ["big"] + SMALL_NAMES)
def test_select_histograms_at_every_shift(w, name):
    c = w.case[name]
    da, db = w.pair(name)
    for alpha, cut_a, cut_b in c.selects:
        for which, with_b in ((0, True), (1, True), (0, False)):
            keys = checker.select_keys(c.a, c.b if with_b else None, alpha, cut_a, cut_b, which, c.unique_shape)
            asks = [(shift, 0, 0) for shift in (range(49) if with_b else (0, 16))]       # (without b: the same loop, one test less)
            if len(keys):
                passes = walk_prefixes(keys, len(keys) // 2)
                asks += passes + [(shift, p, m) for _, p, m in passes[-1:] for shift in (0, 5, 16, 48)]
            for shift, prefix, mask in asks:
                rc, got = hist_call(w, da, db if with_b else None, alpha, cut_a, cut_b, which, shift, prefix, mask)
                want = checker.select_hist(keys, shift, prefix, mask)
                assert rc == 0 and np.array_equal(got, want), (alpha, which, with_b, shift, hex(prefix), hex(mask), int(got.sum()), int(want.sum()))
            rc, again = hist_call(w, da, db if with_b else None, alpha, cut_a, cut_b, which, 0, 0, 0)
            assert rc == 0 and np.array_equal(again, checker.select_hist(keys, 0, 0, 0))               # the same call twice


def test_select_refusals_leave_the_context_working(w):
    from pdb_eda_amd import _native
    c = w.case["tail_1023"]
    da, db = w.pair("tail_1023")
    alpha, cut_a, cut_b = c.selects[0]
    other = w.pair("tail_7")[1]
    for kw in (dict(shift=-1), dict(shift=49), dict(which=2), dict(which=1, b=None), dict(b=other)):
        args = dict(b=db, which=0, shift=0)
        args.update(kw)
        rc, _ = hist_call(w, da, args["b"], alpha, cut_a, cut_b, args["which"], args["shift"], 0, 0)
        assert rc == _native.PDBEDA_ERR_ARGUMENT, kw
    rc, got = hist_call(w, da, db, alpha, cut_a, cut_b, 1, 48, 0, 0)
    assert rc == 0 and np.array_equal(got, checker.select_hist(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 1, c.unique_shape), 48, 0, 0))


# ---- select through Python -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big"] + SMALL_NAMES)
def test_order_statistics_equal_the_sorted_selection(w, name):
    c = w.case[name]
    da, db = w.pair(name)
    for alpha, cut_a, cut_b in c.selects:
        for which in (0, 1):
            keys = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)
            assert da.abs_order_statistics(db, alpha, cut_a, cut_b, which) == len(keys)
            ranks = cases.ranks_of(keys, c.tie_ranks) if len(keys) > 64 else list(range(len(keys)))
            got = da.abs_order_statistics(db, alpha, cut_a, cut_b, which, ranks)
            want = checker.key_values(checker.order_statistics(keys, ranks)).tolist()
            assert [float(x) for x in got] == want, (alpha, which)
        alone = checker.select_keys(c.a, None, alpha, cut_a, cut_b, 0, c.unique_shape)
        assert da.abs_order_statistics(None, 0.0, cut_a, 0.0, 0) == len(alone)
    assert da.abs_order_statistics(db, -2.0, 0.0, 1.0, 0) == 0 and da.abs_order_statistics(db, -2.0, 1.0, 0.0, 1) == 0      # nothing is below 0


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_median_abs_fo_fc_on_tied_maps(w, parity):
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    c = w.case["ties_" + parity]
    fo, diff = (ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(c.spec, g)), "ties", ctx=w.ctx) for g in (c.a, c.b))
    (alpha, cut_a, cut_b), = c.selects
    assert (fo.meanDensity + 1.0 * fo.stdDensity,) * 2 == (cut_a, cut_b)
    want = tuple(float(np.median(checker.key_values(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)))) for which in (0, 1))
    n = len(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 0, c.unique_shape))
    assert n % 2 == (parity == "odd")
    assert densityAnalysis.DensityAnalysis("ties", fo, diff).medianAbsFoFc() == want


# ---- sum_of_abs ------------------------------------------------------------------------------------------------------------------
def sum_cutoffs(c, grid):
    cutoffs = [0.0, -1.0, 0.3, float(np.abs(grid.reshape(-1)[-1])), float(np.abs(grid.reshape(-1)[0]))]
    if c.name == "edges":
        v = cases.CUT_A
        cutoffs += [v, float(np.nextafter(F8(v), F8(0))), float(np.nextafter(F8(v), F8(np.inf))), float(np.nextafter(F4(v), F4(0))), float(np.nextafter(F4(v), F4(2)))]
    return cutoffs


@pytest.mark.parametrize("name", ["big"] + TAIL_NAMES + ["edges"])
def test_sum_of_abs_within_the_bound_of_its_addition_chain(w, name):
    """|got - fsum| <= d * 2^-53 * sum |x| over the voxels that count, d = mapops_cases.sum_chain_depth(n): a value goes through
    4 * trips (+ 1 in a tail lane) additions in its thread of k_reduce_partials, 6 + 4 in block_sum, 8 + 6 + 4 in k_reduce_final --
    d = 41 at 4.25 M voxels, 29 to 33 on the small maps.  Every addition of non-negative terms is off by at most 2^-53 of its result,
    which is at most the whole sum; four of the d additions add to a zero and are exact, which more than pays for the rounding of
    fsum itself and for the second-order terms.  Cutoffs: 0, a negative one, the first and the last voxel's |v| (strict: they
    drop out), and on the edge map a voxel value with the two doubles next to it, which round onto it, and its two float32 neighbours."""
    c = w.case[name]
    da, _ = w.pair(name)
    d = cases.sum_chain_depth(c.n)
    grid = c.a
    if name == "edges":
        assert da.sum_of_abs(0.0) == math.inf == checker.sum_of_abs(c.a, 0.0)                 # the infinities count, the NaNs do not
        grid = cases.finite_part(c.a)
        da = w.device(grid, c)
    lent = Borrowed(w.ctx, grid, c.header.geometry())
    try:
        for cutoff in sum_cutoffs(c, grid):
            want = checker.sum_of_abs(grid, cutoff)
            got = da.sum_of_abs(cutoff)
            print("%s cutoff %r: got %r, fsum %r, |difference| %.3g, bound %.3g (d = %d)" % (name, cutoff, got, want, abs(got - want), d * 2.0 ** -53 * want, d))
            assert abs(got - want) <= d * 2.0 ** -53 * want, cutoff
            assert da.sum_of_abs(cutoff) == got and lent.map.sum_of_abs(cutoff) == got                 # again, and on a buffer of the caller's
    finally:
        lent.free()
        if name == "edges":
            da.free()


# ---- the byte swap of a file upload ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big"] + TAIL_NAMES + ["edges"])
def test_big_endian_file_arrives_as_its_grid(w, tmp_path, name):
    from pdb_eda_amd import _native
    c = w.case[name]
    geom = c.header.geometry()
    swapped = _native.DeviceMap.from_file(w.ctx, big_endian_file(c, c.a, tmp_path / "big_endian.ccp4"), 1024, True, geom)
    plain = _native.DeviceMap.from_file(w.ctx, big_endian_file(c, c.a, tmp_path / "little_endian.ccp4", big_endian=False), 1024, False, geom)
    raw = (tmp_path / "big_endian.ccp4").read_bytes()
    assert np.array_equal(checker.file_grid(raw, 1024, c.a.shape, True).view(np.uint32), c.a.view(np.uint32))
    for m in (swapped, plain):
        assert np.array_equal(m.download().view(np.uint32), c.a.view(np.uint32))              # every voxel, the marked ones and the NaNs included
    assert swapped.__dict__["_file_stats"] is not None
    if name != "edges":                                                                        # (its statistics are NaN)
        da, _ = w.pair(name)
        want = (float(np.mean(c.a, dtype=F8)), float(np.std(c.a.astype(F8))))
        assert swapped.stats() == plain.stats() == da.stats() == want
    swapped.free()
    plain.free()


# ---- which kernels ran at the big size -------------------------------------------------------------------------------------------
def test_profile_names_the_four_kernels_at_the_big_size(w, prof_ctx, tmp_path):
    """On a context of its own, under pdbeda_ctx_profile_begin / _end: one launch each of k_map_combine, k_abs_select_hist,
    k_reduce_partials and k_byteswap32 at 4 251 366 voxels, beyond the first trip of each (mapops_cases.FIRST_TRIP_VOXELS), with the
    results the other context gave."""
    from pdb_eda_amd import _native
    c = w.case["big"]
    assert all(c.n > v for v in cases.FIRST_TRIP_VOXELS.values())
    (alpha, cut_a, cut_b), = c.selects
    path = big_endian_file(c, c.a, tmp_path / "big_endian.ccp4")
    db = w.device(c.b, c, ctx=prof_ctx)
    prof_ctx.profile_begin()
    try:
        da = _native.DeviceMap.from_file(prof_ctx, path, 1024, True, c.header.geometry())
        out = _native.DeviceMap.combine(da, db, alpha)
        count = da.abs_order_statistics(db, alpha, cut_a, cut_b, 1)
        total = da.sum_of_abs(0.0)
    finally:
        prof = prof_ctx.profile_end()
    print("profile at %d voxels: %s" % (c.n, {k: v for k, v in sorted(prof.items())}))
    for kernel in cases.FIRST_TRIP_VOXELS:
        assert prof[kernel][0] == 1, (kernel, prof)
    assert checker.same_bits(out.download(), checker.combine(c.a, c.b, alpha))
    assert count == len(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 1, c.unique_shape))
    assert total == w.pair("big")[0].sum_of_abs(0.0)
    for m in (out, da, db):
        m.free()
