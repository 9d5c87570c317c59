"""The plain numpy restatement of pdbeda_map_spread (include/pdbeda.h): seeds, the per-axis wrap rule, the rank as the FIRST entry of the ordered
table that leads to a seed, the value.  Ranks are painted in DESCENDING t over shifted seed arrays, so the smallest t is what stays -- no rows, no
early exit, nothing the device does.  Grids are [s][r][c]; ``intervals`` is the header's crsInterval, in crs order; offsets are (dc, dr, ds)."""
import numpy as np


def seeds_of(x, threshold, below=False):
    """The seed array: strict comparisons of the float32 voxels widened to fp64 with the float32 threshold widened to fp64; a NaN is no seed."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    t = np.float64(np.float32(threshold))
    with np.errstate(invalid="ignore"):
        return (x < t) if below else (x > t)


def source_index(n, interval, d):
    """idx[i]: the stored index that position i + d reads on one axis, or -1 where it is absent."""
    j = np.arange(n, dtype=np.int64) + int(d)
    outside = (j < 0) | (j >= n)
    j = np.where(outside, j - (j // interval) * interval, j)
    return np.where((j >= n) & (j < interval), -1, j)


def shifted(seed, offset, intervals):
    """out[v] = seed[v + offset] under the wrap rule, False where the position is absent on any axis."""
    out = seed
    ok = np.ones(seed.shape, dtype=bool)
    for crs in range(3):
        axis = 2 - crs
        idx = source_index(seed.shape[axis], intervals[crs], offset[crs])
        out = np.take(out, np.maximum(idx, 0), axis=axis)
        shape = [1, 1, 1]
        shape[axis] = -1
        ok = ok & (idx >= 0).reshape(shape)
    return out & ok


def ranks(x, offsets, intervals, threshold=0.5, below=False):
    """t(v) as int32 [s][r][c]: len(offsets) where no entry leads to a seed."""
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    seed = seeds_of(x, threshold, below)
    t_of = np.full(seed.shape, len(offsets), dtype=np.int32)
    for t in range(len(offsets) - 1, -1, -1):
        t_of[shifted(seed, offsets[t], intervals)] = t
    return t_of


def spread(x, offsets, values, intervals, threshold=0.5, below=False, base=None):
    """pdbeda_map_spread of a float32 grid: float32 [s][r][c]."""
    values = np.asarray(values, dtype=np.float32)
    out = values[ranks(x, offsets, intervals, threshold, below)]
    if base is None:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(base, dtype=np.float32).astype(np.float64) * out.astype(np.float64)).astype(np.float32)


def counters(x, offsets, intervals, threshold=0.5, below=False):
    """(seeds among the stored voxels, voxels with t < n)."""
    return int(seeds_of(x, threshold, below).sum()), int((ranks(x, offsets, intervals, threshold, below) < len(np.asarray(offsets).reshape(-1, 3))).sum())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
