"""CPU: the inputs and the yardsticks of tests/test_gpu_mapops.py (pdbeda_map_combine, pdbeda_abs_select_hist and the digit walk over
it, pdbeda_sum_of_abs, the byte swap of a file upload), checked before a GPU sees them.

tests/mapops_checker.py must equal plain Python loops on the small cases of tests/mapops_cases.py; the product's digit walk
(_native.radix_select), fed with the checker's histograms in place of the device call, must return the sorted keys at every rank of
every case, ties included; every case must have the property it was built for (which side of each kernel's grid cap its size lies on,
the share of ranks inside long runs of equal keys, the occupied bins of the low digits, the planted edge voxels); and per case one
deliberate error -- the last trip of a stride loop dropped, the tail lanes dropped, the stored grid read where the unique box is meant,
<= for <, the byte swap skipped -- must change the checker's answer, so the inputs can see that error."""
import math
import struct

import numpy as np
import pytest

import mapops_cases as cases
import mapops_checker as checker

F4, F8 = np.float32, np.float64


@pytest.fixture(scope="module")
def small():
    return {c.name: c for c in cases.small_cases()}


@pytest.fixture(scope="module")
def big():
    return cases.big()


SMALL_NAMES = ["tail_%d" % n for n in (1, 2, 3, 4, 5, 7, 1023)] + list(cases.GEOMETRY) + ["edges", "ties_even", "ties_odd", "low_digits"]
LOOPED = ["tail_1", "tail_2", "tail_3", "tail_4", "tail_5", "tail_7", "geom_all", "geom_perm", "edges"]      # small enough for Python loops


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def bits32(x):
    return struct.unpack("I", struct.pack("f", x))[0]


def bits64(x):
    return struct.unpack("Q", struct.pack("d", x))[0]


def to_f32(x):
    """A Python double rounded to the nearest float32 (struct refuses what overflows: that is an infinity)."""
    try:
        return f32(x)
    except OverflowError:
        return math.copysign(math.inf, x)


# ---- the checker against loops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LOOPED)
def test_checker_equals_python_loops(small, name):
    c = small[name]
    a, b = c.a.reshape(-1).tolist(), c.b.reshape(-1).tolist()
    for alpha in cases.ALPHAS:
        want = [to_f32(x + alpha * y) for x, y in zip(a, b)]
        got = checker.combine(c.a, c.b, alpha).reshape(-1)
        assert all((math.isnan(w) and math.isnan(g)) or bits32(w) == bits32(g) for w, g in zip(want, got.tolist())), alpha
    us, ur, uc = c.unique_shape
    ns, nr, nc = c.a.shape
    for alpha, cut_a, cut_b in c.selects:
        for which, with_b in ((0, True), (1, True), (0, False)):
            keys = []
            for s in range(us):
                for r in range(ur):
                    for col in range(uc):
                        x, y = a[(s * nr + r) * nc + col], b[(s * nr + r) * nc + col]
                        vc = abs(x + alpha * y) if with_b else 0.0
                        if abs(x) < cut_a and (not with_b or vc < cut_b):
                            keys.append(bits64(vc) if which else bits32(abs(x)))
            got = checker.select_keys(c.a, c.b if with_b else None, alpha, cut_a, cut_b, which, c.unique_shape)
            assert got.tolist() == keys, (alpha, which, with_b)
            for shift, prefix, mask in ((0, 0, 0), (16, 0, 0), (0, keys[0] & 0xffff0000, 0xffff0000) if keys else (0, 0, 0)):
                hist = [0] * 65536
                for k in keys:
                    if k & mask == prefix:
                        hist[(k >> shift) & 0xffff] += 1
                assert checker.select_hist(got, shift, prefix, mask).tolist() == hist
            ranks = cases.ranks_of(got)
            assert checker.order_statistics(got, ranks).tolist() == [sorted(keys)[r] for r in ranks]
    for cutoff in (0.0, -1.0, 0.3, 1.5, 0.1 + 1e-12):
        values = cases.finite_part(c.a).reshape(-1).tolist()
        assert checker.sum_of_abs(cases.finite_part(c.a), cutoff) == math.fsum(abs(v) for v in values if abs(v) > f32(cutoff))


# ---- the product's digit walk over the checker's histograms ----------------------------------------------------------------------
def walk(keys, ranks, trace=None):
    from pdb_eda_amd import _native

    def digit(shift, prefix, mask):
        if trace is not None:
            trace.append((shift, prefix, mask))
        return checker.select_hist(keys, shift, prefix, mask)
    return _native.radix_select(digit, 64 if keys.dtype == np.uint64 else 32, ranks)


def selections(c):
    for alpha, cut_a, cut_b in c.selects:
        for which in (0, 1):
            yield (alpha, cut_a, cut_b, which), checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_digit_walk_returns_the_sorted_keys(small, name):
    c = small[name]
    for what, keys in selections(c):
        ranks = cases.ranks_of(keys, c.tie_ranks)
        if len(keys) <= 64:
            ranks = list(range(len(keys)))                  # every rank of a small selection
        assert walk(keys, ranks) == checker.order_statistics(keys, ranks).tolist(), what


def test_digit_walk_on_the_big_map(big):
    (alpha, cut_a, cut_b), = big.selects
    for which in (0, 1):
        keys = checker.select_keys(big.a, big.b, alpha, cut_a, cut_b, which, big.unique_shape)
        ranks = cases.ranks_of(keys)
        assert walk(keys, ranks) == checker.order_statistics(keys, ranks).tolist()


# ---- each size's side of each kernel's cap ---------------------------------------------------------------------------------------
def test_big_map_turns_every_loop_and_small_maps_none(big, small):
    n = big.n
    assert n == 4251366 and n % 4 == 2 and big.unique_shape == big.a.shape
    assert cases.FIRST_TRIP_VOXELS == {"k_abs_select_hist": 1048576, "k_map_combine": 4194304, "k_reduce_partials": 2097152, "k_byteswap32": 2097152}
    assert all(n > v for v in cases.FIRST_TRIP_VOXELS.values())
    loops = {"k_abs_select_hist": (n, cases.select_threads(n)), "k_map_combine": (n // 4, cases.combine_threads(n)),
             "k_reduce_partials": (n // 4, cases.reduce_threads(n)), "k_byteswap32": (n, cases.swap_threads(n))}
    assert {k: cases.trips(*v) for k, v in loops.items()} == {"k_abs_select_hist": 5, "k_map_combine": 2, "k_reduce_partials": 3, "k_byteswap32": 3}
    per_item = {"k_abs_select_hist": 1, "k_map_combine": 4, "k_reduce_partials": 4, "k_byteswap32": 1}
    for k, (items, threads) in loops.items():            # the last trip of every loop starts at voxel 4 194 304, a marked one
        assert (cases.trips(items, threads) - 1) * threads * per_item[k] == cases.BIG_MARKED[0], k
    assert cases.BIG_MARKED[1:] == (n - 3, n - 2, n - 1)
    for c in small.values():
        u = int(np.prod(c.unique_shape))
        assert cases.trips(u, cases.select_threads(u)) == 1 and cases.trips(c.n // 4, cases.combine_threads(c.n)) <= 1
        assert cases.trips(c.n // 4, cases.reduce_threads(c.n)) <= 1 and cases.trips(c.n, cases.swap_threads(c.n)) == 1
    assert cases.sum_chain_depth(n) == 41 and cases.sum_chain_depth(7) == 33 and cases.sum_chain_depth(3) == 29


def test_big_map_markers_and_dropped_trips(big):
    """The marked voxels hold values found nowhere else, the select keeps them, and a loop without its last trip (or a kernel without its
    tail lanes) gives another answer from every operation."""
    n = big.n
    a, b = big.a.reshape(-1), big.b.reshape(-1)
    (alpha, cut_a, cut_b), = big.selects
    for at in cases.BIG_MARKED:
        assert np.count_nonzero(np.abs(a) == abs(a[at])) == 1 and np.count_nonzero(np.abs(b) == abs(b[at])) == 1
        assert abs(float(a[at])) < cut_a and abs(float(a[at]) + alpha * float(b[at])) < cut_b
    want = checker.combine(a, b, alpha)
    # combine and the reduction: float4 items, and n % 4 tail lanes
    for threads in (cases.combine_threads(n), cases.reduce_threads(n)):
        kept = np.repeat(checker.loop_cover(n // 4, threads, drop_last_trip=True), 4)
        assert kept.sum() == cases.BIG_MARKED[0] and not kept[cases.BIG_MARKED[0]]
        kept = np.concatenate((kept, np.ones(n % 4, dtype=bool)))
        assert not np.array_equal(np.where(kept, want, 0), want)
        total = checker.sum_of_abs(a, 0.0)
        for missing in (~kept, np.arange(n) >= n - n % 4):                     # the last trip; the tail lanes
            assert abs(checker.sum_of_abs(np.where(missing, 0, a), 0.0) - total) > 1e3 * cases.sum_chain_depth(n) * 2.0 ** -53 * total
    keys = checker.select_keys(big.a, big.b, alpha, cut_a, cut_b, 0, big.unique_shape)
    kept = checker.loop_cover(n, cases.select_threads(n), drop_last_trip=True)
    fewer = checker.select_keys(np.where(kept, a, np.inf).reshape(big.a.shape), big.b, alpha, cut_a, cut_b, 0, big.unique_shape)
    assert 0 < len(keys) - len(fewer) and 200000 < len(keys) < n // 2
    assert not np.array_equal(checker.select_hist(keys, 0, 0, 0), checker.select_hist(fewer, 0, 0, 0))
    # the file upload: a swap that stops before its last trip, or does not happen
    raw = np.ascontiguousarray(big.a.astype(">f4")).tobytes()
    assert np.array_equal(checker.file_grid(raw, 0, big.a.shape, True).view(np.uint32), big.a.view(np.uint32))
    unswapped = checker.file_grid(raw, 0, big.a.shape, False).reshape(-1)
    kept = checker.loop_cover(n, cases.swap_threads(n), drop_last_trip=True)
    for wrong in (unswapped, np.where(kept, a, unswapped)):
        assert not np.array_equal(wrong.view(np.uint32), a.view(np.uint32))
        with np.errstate(all="ignore"):
            assert float(np.mean(wrong, dtype=F8)) != float(np.mean(a, dtype=F8))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023])
def test_tail_shapes(small, n):
    """n % 4 in 0..3 with n / 4 in {0, 1, many}; without its tail lanes (or, where there are none, without its only trip) every operation
    gives another answer."""
    c = small["tail_%d" % n]
    assert c.n == n and c.unique_shape == c.a.shape
    assert sorted({(m % 4, min(m // 4, 2)) for m in (1, 2, 3, 4, 5, 7, 1023)}) == [(0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1), (3, 2)]
    a = c.a.reshape(-1)
    missing = np.arange(n) >= (n - n % 4 if n % 4 else 0)
    assert np.all(a[missing] != 0) and np.all(checker.combine(c.a, c.b, -2.0).reshape(-1)[missing] != 0)
    assert checker.sum_of_abs(np.where(missing, 0, a), 0.0) != checker.sum_of_abs(a, 0.0)
    alpha, cut_a, cut_b = c.selects[-1]                     # infinite cuts: every voxel selected, the last one too
    assert len(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 1, c.unique_shape)) == n
    raw = np.ascontiguousarray(c.a.astype(">f4")).tobytes()
    assert not np.array_equal(checker.file_grid(raw, 0, c.a.shape, False).view(np.uint32), c.a.view(np.uint32))


# ---- geometry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GEOMETRY))
def test_unique_box_cases_see_a_leak(small, name):
    from pdb_eda_amd import _native
    c = small[name]
    assert c.unique_shape == cases.GEOMETRY_UNIQUE[name] and c.unique_shape != c.a.shape
    g = c.header.geometry()
    assert tuple(min(g.ncrs[k], g.xyz_interval[g.map2crs[k]]) for k in (2, 1, 0)) == c.unique_shape      # DeviceMap.unique_shape
    us, ur, uc = c.unique_shape
    inside = np.zeros(c.a.shape, dtype=bool)
    inside[:us, :ur, :uc] = True
    for alpha, cut_a, cut_b in c.selects:
        for grid in (np.abs(c.a.astype(F8)), np.abs(c.a.astype(F8) + alpha * c.b.astype(F8))):
            assert np.all(grid[~inside] < min(cut_a, cut_b)) and not np.intersect1d(grid[~inside], grid[inside]).size
        for which in (0, 1):
            keys = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)
            leaked = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape, mutate="stored")
            assert 0 < len(keys) < inside.sum() and len(leaked) == len(keys) + (~inside).sum()
            assert not np.array_equal(checker.select_hist(keys, 48 * which + 16 * (1 - which), 0, 0), checker.select_hist(leaked, 48 * which + 16 * (1 - which), 0, 0))
    if name == "geom_perm":                                  # the interval taken in crs order would be another box
        assert tuple(min(g.ncrs[k], g.xyz_interval[k]) for k in (2, 1, 0)) != c.unique_shape


# ---- value edges -----------------------------------------------------------------------------------------------------------------
def test_edge_voxels_are_where_they_were_planted(small):
    c = small["edges"]
    plants = cases.edge_plants()
    a, b = c.a.reshape(-1), c.b.reshape(-1)
    assert c.n == 3553 and c.n % 4 == 1 and abs(float(a[-1])) == cases.CUT_A and abs(float(a[0])) == cases.CUT_A

    def where(pairs):
        out = []
        for pa, pb in pairs:
            hit = np.flatnonzero((a.view(np.uint32) == F4(pa).view(np.uint32)) & (b.view(np.uint32) == F4(pb).view(np.uint32)))
            assert len(hit) >= 1, (pa, pb)
            out.extend(hit.tolist())
        return np.array(out)
    at = {k: where(v) for k, v in plants.items()}
    sub = np.abs(a[at["subnormal"]])
    assert np.count_nonzero((sub > 0) & (sub < np.finfo(F4).tiny)) >= 6
    for alpha, cut_a, cut_b in c.selects[:2]:
        with np.errstate(all="ignore"):
            vc = np.abs(a.astype(F8) + alpha * b.astype(F8))
            keep = (np.abs(a.astype(F8)) < cut_a) & (vc < cut_b)
        assert cut_b == cases.cut_b_of(alpha) and np.all(vc[at["on_cut_b"]] == cut_b) and np.all(np.abs(a[at["on_cut_a"]]) == cut_a)
        assert not keep[at["on_cut_a"]].any() and not keep[at["on_cut_b"]].any() and not keep[at["outside_cut_a"]].any() and not keep[at["nonfinite"]].any()
        assert keep[at["inside_cut_a"]].sum() >= 2 and keep[at["inside_cut_b"]].all() and keep[at["zeros"]].all() and keep[at["pairs"]].all()
        assert np.count_nonzero(vc[at["on_cut_a"]] < cut_b) >= 2          # <= on the first cut would let these in
        for which in (0, 1):
            keys = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)
            loose = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape, mutate="le")
            assert len(loose) >= len(keys) + 6 and np.count_nonzero(keys == 0) >= 4                # (+0 and -0: one key)
    for alpha, cut_a, cut_b in c.selects[2:]:                               # infinite cuts: what is finite in a and in a + alpha b
        with np.errstate(all="ignore"):
            finite = np.isfinite(a) & np.isfinite(a.astype(F8) + alpha * b.astype(F8))
        assert len(checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 1, c.unique_shape)) == finite.sum() == c.n - len(plants["nonfinite"])
        assert len(checker.select_keys(c.a, None, alpha, cut_a, cut_b, 0, c.unique_shape)) == np.isfinite(a).sum() > finite.sum()
    # combine: subnormal results from normal operands, infinities from finite ones
    for alpha in cases.ALPHAS:
        out = checker.combine(a, b, alpha)
        finite_in = np.isfinite(a) & np.isfinite(b)
        tiny = (out != 0) & (np.abs(out) < np.finfo(F4).tiny)
        assert tiny.sum() >= 4 and (np.isinf(out) & finite_in).sum() >= (2 if alpha else 0)
    assert (np.abs(checker.combine(a, b, -2.0)) < np.finfo(F4).tiny)[np.abs(a) >= np.finfo(F4).tiny].any()
    # sum_of_abs: strict at a cutoff that is a voxel's value, and a double cutoff that rounds onto that value from either side
    fin = cases.finite_part(c.a)
    assert math.isinf(checker.sum_of_abs(c.a, 0.0)) and math.isfinite(checker.sum_of_abs(fin, 0.0)) and np.isnan(fin).sum() == 2
    u, v, w = (float(np.nextafter(F4(cases.CUT_A), F4(0))), cases.CUT_A, float(np.nextafter(F4(cases.CUT_A), F4(2))))
    assert all(np.count_nonzero(np.abs(fin) == F4(x)) >= 4 for x in (u, v, w))
    assert checker.sum_of_abs(fin, v) != checker.sum_of_abs(fin, v, mutate="ge")
    for cutoff in sum_cutoffs_across(v):
        assert F4(cutoff) == F4(v) and cutoff != v
        assert checker.sum_of_abs(fin, cutoff) == checker.sum_of_abs(fin, v)
    below, above = sum_cutoffs_across(v)
    assert checker.sum_of_abs(fin, below, mutate="double_cutoff") > checker.sum_of_abs(fin, below)            # the unrounded cutoff lets v in
    # (a cutoff rounded up instead of to nearest would be w for `above` and leave the voxels at w out)
    assert checker.sum_of_abs(fin, w) < checker.sum_of_abs(fin, above)


def sum_cutoffs_across(v):
    """Two Python doubles next to the float32 value v, one on either side, that round to v."""
    return float(np.nextafter(F8(v), F8(0))), float(np.nextafter(F8(v), F8(np.inf)))


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def lower_bound_walk(keys, ranks):
    """The digit walk with its one decision mutated: the first bin whose cumulated count reaches the rank, where the product takes the
    first that exceeds it."""
    out = []
    for rank in ranks:
        prefix, mask, remaining = 0, 0, int(rank)
        for shift in range(keys.dtype.itemsize * 8 - 16, -1, -16):
            cs = np.cumsum(checker.select_hist(keys, shift, prefix, mask))
            d = min(int(np.searchsorted(cs, remaining, side="left")), 65535)
            remaining -= int(cs[d - 1]) if d else 0
            prefix |= d << shift
            mask |= 0xffff << shift
        out.append(prefix)
    return out



@pytest.mark.parametrize("parity", [0, 1])
def test_tie_cases_ask_inside_long_runs(small, parity):
    c = small["ties_odd" if parity else "ties_even"]
    assert len(np.unique(np.abs(c.a))) == 41
    (alpha, cut_a, cut_b), = c.selects
    assert (cut_a, cut_b) == cases.median_cuts(c.a) and alpha == -2.0
    for which in (0, 1):
        keys = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, which, c.unique_shape)
        n = len(keys)
        assert n % 2 == parity and n > 3000
        ranks = cases.ranks_of(keys, ties=True)
        first, length = cases.largest_run(keys)
        assert {0, n - 1, n // 2, first, first + length - 1} <= set(ranks) and (parity or n // 2 - 1 in ranks)
        starts, lengths = cases.runs(keys)
        inside = 0
        for r in ranks:
            k = int(np.searchsorted(starts, r, side="right")) - 1
            inside += lengths[k] >= 100 and starts[k] < r < starts[k] + lengths[k] - 1
        assert 2 * inside >= len(ranks), (inside, len(ranks))
        assert walk(keys, ranks) == checker.order_statistics(keys, ranks).tolist()
        assert lower_bound_walk(keys, ranks) != checker.order_statistics(keys, ranks).tolist()         # a walk that breaks ties the other way shows here
        # the median that medianAbsFoFc reports
        mid = [n // 2] if n % 2 else [n // 2 - 1, n // 2]
        assert float(np.mean(checker.key_values(checker.order_statistics(keys, mid)))) == float(np.median(checker.key_values(keys)))


# ---- low digits ------------------------------------------------------------------------------------------------------------------
def test_low_digit_case_fills_the_low_histograms(small):
    c = small["low_digits"]
    (alpha, cut_a, cut_b), (alpha2, _, _) = c.selects
    assert alpha == math.sqrt(0.5) and alpha2 == -2.0
    keys = checker.select_keys(c.a, c.b, alpha, cut_a, cut_b, 1, c.unique_shape)
    assert np.count_nonzero(checker.select_hist(keys, 0, 0, 0)) >= 1000 and np.count_nonzero(checker.select_hist(keys, 16, 0, 0)) >= 1000
    product = checker.select_keys(c.a, c.b, alpha2, c.selects[1][1], c.selects[1][2], 1, c.unique_shape)
    assert np.count_nonzero(checker.select_hist(product, 0, 0, 0)) < 10          # what alpha = -2 leaves of the lowest digit
    ranks = cases.ranks_of(keys)
    got = walk(keys, ranks)
    assert got == checker.order_statistics(keys, ranks).tolist()
    assert any((k & 0xffff) and ((k >> 16) & 0xffff) for k in got)
    trace = []
    walk(keys, ranks[:1], trace)
    assert [t[0] for t in trace] == [48, 32, 16, 0] and trace[-1][2] == 0xffffffffffff0000
