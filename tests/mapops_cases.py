"""Seeded inputs of tests/test_mapops_host.py and tests/test_gpu_mapops.py: pairs of maps (a, b) for pdbeda_map_combine,
pdbeda_abs_select_hist (with the digit walk of DeviceMap.abs_order_statistics), pdbeda_sum_of_abs and the byte swap of a file upload.
Each case is the smallest that turns a loop or takes a branch; tests/test_mapops_host.py shows on the CPU that it does.

big()          161 x 163 x 162 = 4 251 366 voxels (n % 4 = 2): every stride loop below turns, the last trip of each starts at voxel
               4 194 304; that voxel and the last three hold marker values that occur nowhere else and pass the select's cuts.
tails()        (1, 1, n) for n = 1, 2, 3, 4, 5, 7 and (1, 3, 341): n % 4 = 0..3 with n / 4 = 0, 1 and many.
geometry()     ncrs (13, 11, 9) with the cell's interval below ncrs on c, on r, on s, on all three, and on all three under a
               permuted axis order; outside the unique box lie magnitudes that pass both cuts and occur nowhere inside it.
edges()        3 553 voxels with planted voxels on either cut, one float32 ulp inside it, +-0, pairs +-v, NaN, +-inf, float32
               subnormals and sums beyond the float32 range.
ties(parity)   10 080 voxels quantised to 41 magnitudes; the selection of DensityAnalysis.medianAbsFoFc holds an odd / even count.
low_digits()   the two 27 930-voxel maps of test_map_combine_download_and_order_statistics with alpha = sqrt(0.5) and with -2.

The launch lines the caps are taken from (pdb_eda_amd/csrc/pdbeda_hip.hip):
  pdbeda_abs_select_hist   k_abs_select_hist <<< grid_for(n_unique, 256, 4096), 256 >>>     one voxel a thread and trip
  pdbeda_map_combine       k_map_combine     <<< grid_for(n / 4 + 1, 256, 4096), 256 >>>     one float4 a thread and trip, n % 4 tail lanes
  reduce_launch            k_reduce_partials <<< N_PARTIAL = 2048, 256 >>>                   one float4 a thread and trip, n % 4 tail lanes
  upload_file_impl         k_byteswap32      <<< grid_for(n, 256, 8192), 256 >>>             one voxel a thread and trip"""
import math

import numpy as np

F4, F8 = np.float32, np.float64
SQRT_HALF = math.sqrt(0.5)
ALPHAS = (-2.0, 1.0, 0.0, SQRT_HALF)          # combine; the select uses the first and the last

BLOCK = 256
SELECT_CAP, COMBINE_CAP, N_PARTIAL, SWAP_CAP = 4096, 4096, 2048, 8192


def grid_for(n, block, cap):
    return max(1, min((n + block - 1) // block, cap))


def select_threads(n_unique):
    return grid_for(n_unique, BLOCK, SELECT_CAP) * BLOCK


def combine_threads(n):
    return grid_for(n // 4 + 1, BLOCK, COMBINE_CAP) * BLOCK


def reduce_threads(n):
    return N_PARTIAL * BLOCK


def swap_threads(n):
    return grid_for(n, BLOCK, SWAP_CAP) * BLOCK


def trips(n_items, n_threads):
    return -(-n_items // n_threads)


# voxels beyond which a kernel's loop takes a second trip
FIRST_TRIP_VOXELS = {"k_abs_select_hist": SELECT_CAP * BLOCK, "k_map_combine": 4 * COMBINE_CAP * BLOCK, "k_reduce_partials": 4 * N_PARTIAL * BLOCK,
                     "k_byteswap32": SWAP_CAP * BLOCK}


def sum_chain_depth(n):
    """The longest chain of fp64 additions that one voxel's |v| passes through in pdbeda_sum_of_abs (pdbeda_kernels.h):
    k_reduce_partials  a thread adds four values a trip of its float4 loop, ceil((n / 4) / (2048 * 256)) trips at the most, and a tail lane
                       one value more;
    block_sum          six __shfl_down steps (32 .. 1), then thread 0 adds the four waves' sums to 0;
    k_reduce_final     a thread adds 2048 / 256 = 8 partials, and block_sum again."""
    return 4 * trips(n // 4, reduce_threads(n)) + 1 + (6 + 4) + N_PARTIAL // BLOCK + (6 + 4)


class Case(object):
    def __init__(self, name, spec, a, b, selects, tie_ranks=False):
        self.name, self.spec, self.a, self.b = name, spec, a, b
        self.selects = selects            # [(alpha, cut_a, cut_b)]
        self.tie_ranks = tie_ranks

    @property
    def header(self):
        from pdb_eda_amd import ccp4, synthetic
        return ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(self.spec))

    @property
    def unique_shape(self):
        return tuple(self.header.uniqueNcrs[::-1])

    @property
    def n(self):
        return self.a.size


def spec_of(shape, **kw):
    from pdb_eda_amd import synthetic
    return synthetic.MapSpec(ncrs=tuple(shape[::-1]), **kw)


def ranks_of(keys, ties=False):
    """0, n - 1 and the middle rank(s); with ties also the first and the last rank of the largest run of equal keys, its middle, and
    three ranks in between."""
    n = len(keys)
    if n == 0:
        return []
    ranks = [0, n - 1] + ([n // 2] if n % 2 else [n // 2 - 1, n // 2])
    if ties:
        first, length = largest_run(keys)
        ranks += [first, first + length - 1, first + length // 2, n // 4, n // 3, (3 * n) // 4]
    return ranks


def runs(keys):
    """(first rank, length) of every run of equal keys in the ascending order."""
    s = np.sort(keys)
    starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
    return starts, np.diff(np.concatenate((starts, [len(s)])))


def largest_run(keys):
    starts, lengths = runs(keys)
    k = int(np.argmax(lengths))
    return int(starts[k]), int(lengths[k])


# ---- 1. the big map -------------------------------------------------------------------------------------------------------------
BIG_SHAPE = (162, 163, 161)
BIG_MARKED = (4194304, 4251363, 4251364, 4251365)


def big():
    rng = np.random.default_rng(101)
    a = rng.standard_normal(BIG_SHAPE, dtype=F4)
    b = rng.standard_normal(BIG_SHAPE, dtype=F4) * F4(0.5)
    for k, at in enumerate(BIG_MARKED):            # dyadic markers inside both cuts: 2^-6 (1 + k / 8), the sign alternating
        a.reshape(-1)[at] = F4((1 + k / 8) / 64 * (-1) ** k)
        b.reshape(-1)[at] = F4((k + 1) / 1024)
    return Case("big", spec_of(BIG_SHAPE), a, b, [(-2.0, 0.4, 0.8)])


# ---- 2. tails -------------------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (1, 1, 5), (1, 1, 7), (1, 3, 341)]


def tails():
    out = []
    for shape in TAIL_SHAPES:
        n = int(np.prod(shape))
        rng = np.random.default_rng(200 + n)
        a = (rng.standard_normal(shape) * 0.6).astype(F4)
        b = (rng.standard_normal(shape) * 0.3).astype(F4)
        out.append(Case("tail_%d" % n, spec_of(shape), a, b, [(-2.0, 1.0, 1.2), (SQRT_HALF, 1.0, 1.2), (-2.0, np.inf, np.inf)]))
    return out


# ---- 3. repeating and permuted geometry -----------------------------------------------------------------------------------------
GEOMETRY = {"geom_c": dict(interval=(7, 11, 9)), "geom_r": dict(interval=(13, 6, 9)), "geom_s": dict(interval=(13, 11, 5)),
            "geom_all": dict(interval=(7, 6, 5)),
            # columns run along Y, rows along Z, sections along X: unique ncrs = (min(13, 7), min(11, 6), min(9, 5)), while the
            # interval read in crs order would give (5, 7, 6)
            "geom_perm": dict(interval=(5, 7, 6), axis_order=(2, 3, 1))}
GEOMETRY_UNIQUE = {"geom_c": (9, 11, 7), "geom_r": (9, 6, 13), "geom_s": (5, 11, 13), "geom_all": (5, 6, 7), "geom_perm": (5, 6, 7)}


def geometry():
    out = []
    for k, (name, kw) in enumerate(GEOMETRY.items()):
        shape = (9, 11, 13)
        rng = np.random.default_rng(300 + k)
        sign = lambda: rng.choice(np.array([-1.0, 1.0]), shape)
        us, ur, uc = GEOMETRY_UNIQUE[name]
        inside = np.zeros(shape, dtype=bool)
        inside[:us, :ur, :uc] = True
        # inside the box magnitudes of [0.125, 1), outside of (0, 0.0625): all of those pass the cuts, and none occurs inside
        a = np.where(inside, rng.uniform(0.125, 1.0, shape), rng.uniform(0.001, 0.0625, shape)) * sign()
        b = np.where(inside, rng.uniform(0.125, 0.5, shape), rng.uniform(0.0001, 0.001, shape)) * sign()
        out.append(Case(name, spec_of(shape, **kw), a.astype(F4), b.astype(F4), [(-2.0, 0.9, 1.1), (SQRT_HALF, 0.9, 1.1)]))
    return out


# ---- 4. value edges -------------------------------------------------------------------------------------------------------------
EDGE_SHAPE = (11, 17, 19)
CUT_A = 1.5
ON_CUT_B = (1.0, 0.125)                   # |a + alpha b| of this pair IS the second cut of the select with that alpha


def cut_b_of(alpha):
    return abs(F8(ON_CUT_B[0]) + F8(alpha) * F8(ON_CUT_B[1]))


def edge_plants():
    """{what: [(a, b)]} -- what edges() writes over its noise."""
    inf, nan = np.inf, np.nan
    lo = lambda v: float(np.nextafter(F4(v), F4(0)))
    hi = lambda v: float(np.nextafter(F4(v), F4(np.inf)))
    sub = float(np.nextafter(F4(0), F4(1)))                  # the smallest float32 subnormal
    pm = lambda pairs: [p for a, b in pairs for p in ((a, b), (-a, -b))]
    return {
        "on_cut_a": pm([(CUT_A, 0.5), (CUT_A, -1.0)]),                                # b chosen so that each passes the second cut with one of the alphas
        "inside_cut_a": pm([(lo(CUT_A), 0.5), (lo(CUT_A), -1.0)]),
        "outside_cut_a": pm([(hi(CUT_A), 0.5), (hi(CUT_A), -1.0)]),
        "on_cut_b": pm([ON_CUT_B, ON_CUT_B]),
        "inside_cut_b": pm([(lo(ON_CUT_B[0]), ON_CUT_B[1])]),
        "zeros": [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)],
        "pairs": pm([(0.375, 0.0625), (0.71875, 0.21875), (0.0078125, 0.25)]),
        "nonfinite": [(nan, 0.1), (0.1, nan), (inf, 0.1), (-inf, 0.1), (0.1, inf), (0.1, -inf), (nan, nan), (inf, inf), (inf, -inf)],
        "subnormal": pm([(1e-40, 3e-41), (sub, 0.0), (0.0, sub), (sub, sub), (1e-38, -5e-39), (2e-38, 1e-38), (1e-40, 0.25)]),
        "overflow": pm([(3e38, -3e38), (3.4e38, 3.4e38), (3.4e38, 1e38)]),
    }


def edges():
    rng = np.random.default_rng(400)
    a = (rng.standard_normal(EDGE_SHAPE) * 0.5).astype(F4).reshape(-1)
    b = (rng.standard_normal(EDGE_SHAPE) * 0.3).astype(F4).reshape(-1)
    plants = [p for group in edge_plants().values() for p in group]
    # scattered, but the last voxel (the tail lane: 3 553 % 4 = 1) and voxel 0 hold planted ones: a voxel on the first cut each
    at = np.concatenate(([a.size - 1, 0], rng.permutation(np.arange(1, a.size - 1))[:len(plants) - 2]))
    for k, (pa, pb) in zip(at, plants):
        a[k], b[k] = F4(pa), F4(pb)
    selects = [(-2.0, CUT_A, cut_b_of(-2.0)), (SQRT_HALF, CUT_A, cut_b_of(SQRT_HALF)), (-2.0, np.inf, np.inf), (SQRT_HALF, np.inf, np.inf)]
    return Case("edges", spec_of(EDGE_SHAPE), a.reshape(EDGE_SHAPE), b.reshape(EDGE_SHAPE), selects)


def finite_part(grid):
    """The grid with its infinities, and the values near the float32 maximum, replaced by +-2.5 (the NaNs stay): sum_of_abs is then
    finite, and a voxel of ordinary size still shows in it."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(grid) > 1e30, np.copysign(F4(2.5), grid), grid).astype(F4)


# ---- 5. ties --------------------------------------------------------------------------------------------------------------------
TIE_SHAPE = (12, 21, 40)


def median_cuts(a):
    """foCut = fcCut of DensityAnalysis.medianAbsFoFc: mean + 1 sigma of the Fo map, numpy's."""
    cut = float(np.mean(a, dtype=F8)) + 1.0 * float(np.std(a.astype(F8)))
    return cut, cut


def ties(parity):
    """a in k / 32, b in k / 64: 41 magnitudes of |a| and few more of |a - 2 b|.  The first seed whose medianAbsFoFc selection has the
    asked parity (0 even, 1 odd)."""
    from mapops_checker import select_keys
    for seed in range(500, 540):
        rng = np.random.default_rng(seed)
        a = (rng.integers(-40, 41, TIE_SHAPE) / 32.0).astype(F4)
        b = (rng.integers(-8, 9, TIE_SHAPE) / 64.0).astype(F4)
        cut_a, cut_b = median_cuts(a)
        if len(select_keys(a, b, -2.0, cut_a, cut_b, 0, TIE_SHAPE)) % 2 == parity:
            return Case("ties_%s" % ("odd" if parity else "even"), spec_of(TIE_SHAPE), a, b, [(-2.0, cut_a, cut_b)], tie_ranks=True)
    raise AssertionError("no seed gives that parity")


# ---- 6. low digits of the 64-bit key --------------------------------------------------------------------------------------------
def low_digits():
    from pdb_eda_amd import synthetic
    shape = (21, 19, 70)
    a, b = synthetic.smooth_noise(shape, 41, 1.2), synthetic.smooth_noise(shape, 42, 1.0)
    cut_a = float(np.abs(a).mean() * 1.3)
    selects = [(alpha, cut_a, float(np.abs(a.astype(F8) + alpha * b.astype(F8)).mean() * 1.1)) for alpha in (SQRT_HALF, -2.0)]
    return Case("low_digits", spec_of(shape), a, b, selects)


def small_cases():
    """Every case but the big one."""
    return tails() + geometry() + [edges(), ties(0), ties(1), low_digits()]
