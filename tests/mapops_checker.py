"""The small whole-map operations restated in numpy, fp64: pdbeda_map_combine, pdbeda_abs_select_hist with the order statistics its
digit walk leads to, pdbeda_sum_of_abs, and the byte swap of a file upload.  Nothing here knows how a kernel walks a grid; what a
kernel's loop covers is modelled apart (``loop_cover``), for the mutation checks of tests/test_mapops_host.py.

``mutate`` names one deliberate error, for those checks only: "stored" (the stored grid where the unique box is meant), "le" (<= where
the cuts are strict), "ge" (>= where sum_of_abs is strict), "double_cutoff" (the cutoff of sum_of_abs not rounded to float32)."""
import math

import numpy as np

F4, F8 = np.float32, np.float64


def combine(a, b, alpha):
    """float32(double(a) + alpha * double(b)): two fp64 roundings, then one to float32."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, dtype=F4).astype(F8) + F8(alpha) * np.asarray(b, dtype=F4).astype(F8)).astype(F4)


def select_keys(a, b, alpha, cut_a, cut_b, which, unique_shape, mutate=None):
    """The keys (uint32 for which = 0, uint64 for which = 1) of the voxels of the unique box a[:us, :ur, :uc] with |a| < cut_a and, when
    b is given, |a + alpha b| < cut_b, in grid order.  Strict comparisons of fp64 magnitudes: a NaN fails them."""
    assert which in (0, 1) and (which == 0 or b is not None)
    us, ur, uc = a.shape if mutate == "stored" else unique_shape
    a32 = np.ascontiguousarray(np.asarray(a, dtype=F4)[:us, :ur, :uc]).reshape(-1)
    below = (lambda x, cut: x <= cut) if mutate == "le" else (lambda x, cut: x < cut)
    with np.errstate(all="ignore"):
        keep = below(np.abs(a32.astype(F8)), F8(cut_a))
        vc = np.zeros(a32.size, dtype=F8)
        if b is not None:
            b32 = np.ascontiguousarray(np.asarray(b, dtype=F4)[:us, :ur, :uc]).reshape(-1)
            vc = np.abs(a32.astype(F8) + F8(alpha) * b32.astype(F8))
            keep &= below(vc, F8(cut_b))
    if which:
        return np.ascontiguousarray(vc[keep]).view(np.uint64)
    return np.ascontiguousarray(np.abs(a32[keep])).view(np.uint32)


def select_hist(keys, shift, prefix, mask):
    """65536 bins of bits [shift, shift + 16) of the keys that agree with ``prefix`` on ``mask``."""
    k = keys.astype(np.uint64)
    k = k[(k & np.uint64(mask)) == np.uint64(prefix)]
    return np.bincount(((k >> np.uint64(shift)) & np.uint64(0xffff)).astype(np.int64), minlength=65536).astype(np.int64)


def key_values(keys):
    """The magnitudes that keys stand for, as float64."""
    return keys.view(F4).astype(F8) if keys.dtype == np.uint32 else keys.view(F8)


def order_statistics(keys, ranks):
    """The keys at the 0-based ranks of the ascending order (the order of the keys is the order of the magnitudes)."""
    return np.sort(keys)[np.asarray(ranks, dtype=np.int64)]


def sum_of_abs(grid, cutoff, mutate=None):
    """sum |v| over |v| > float32(cutoff), strict, correctly rounded (math.fsum).  A NaN is greater than nothing."""
    a = np.abs(np.asarray(grid, dtype=F4).astype(F8)).reshape(-1)
    c = F8(cutoff) if mutate == "double_cutoff" else F8(F4(cutoff))
    with np.errstate(invalid="ignore"):
        keep = a >= c if mutate == "ge" else a > c
    return math.fsum(a[keep].tolist())


def file_grid(raw, offset, shape, swapped):
    """The float32 grid that a file upload must leave in memory: the bytes behind ``offset`` read in this machine's byte order, every
    32-bit word reversed when the file has the other one."""
    words = np.frombuffer(raw, dtype=np.uint32, count=int(np.prod(shape)), offset=offset)
    return (words.byteswap() if swapped else words).view(F4).reshape(shape)


def loop_cover(n_items, n_threads, drop_last_trip=False):
    """Which of n_items a grid-stride loop of n_threads threads visits (all of them), or what is left when its last trip is dropped."""
    covered = np.ones(n_items, dtype=bool)
    if drop_last_trip and n_items:
        covered[(-(-n_items // n_threads) - 1) * n_threads:] = False
    return covered


def same_bits(got, want):
    """float32 arrays equal as uint32, except that a NaN only has to be a NaN: IEEE 754 leaves the sign and the payload of a NaN that an
    operation makes (inf - inf, 0 * inf) to the implementation, and the host and the device choose differently."""
    got, want = np.asarray(got, dtype=F4).reshape(-1), np.asarray(want, dtype=F4).reshape(-1)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
