"""The plain numpy restatement of pdbeda_map_filter and pdbeda_map_local_stats (include/pdbeda.h): the index rule, the tap order, W and
the local formulas.  Every product and every sum is a numpy float64 operation of its own, so nothing is fused and the device, built with
-ffp-contract=off, can be held to these bits.  Grids are [s][r][c]; ``intervals`` is the header's crsInterval, in crs order."""
import numpy as np


def source_index(n, interval, radius):
    """idx[i][k]: the stored index that x~[i + k - radius] reads, or -1 where it is absent (the wrap rule, on one axis)."""
    j = np.arange(n, dtype=np.int64)[:, None] + np.arange(-radius, radius + 1, dtype=np.int64)[None, :]
    outside = (j < 0) | (j >= n)
    j = np.where(outside, j - (j // interval) * interval, j)          # (numpy's // floors, like Python's)
    return np.where((j >= n) & (j < interval), -1, j)


def axis_weights(w, n, interval):
    """W_axis[i] = sum_k w[k + R] * present(i + k), from +0.0 in ascending k."""
    w = np.asarray(w, dtype=np.float64)
    idx = source_index(n, interval, len(w) // 2)
    acc = np.zeros(n, dtype=np.float64)
    for k in range(len(w)):
        acc = acc + w[k] * (idx[:, k] >= 0).astype(np.float64)
    return acc


def filter_axis(x, w, axis, interval):
    """One pass over a float64 array along numpy axis ``axis``."""
    w = np.asarray(w, dtype=np.float64)
    x = np.moveaxis(x, axis, -1)
    idx = source_index(x.shape[-1], interval, len(w) // 2)
    acc = np.zeros(x.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(w)):
            xs = np.where(idx[:, k] >= 0, x[..., np.maximum(idx[:, k], 0)], 0.0)
            acc = acc + w[k] * xs
    return np.moveaxis(acc, -1, axis)


def filter3(x, taps, intervals):
    """F[x]: the passes along c, r and s (numpy axes 2, 1, 0) in that order, fp64 throughout, not rounded."""
    y = np.asarray(x, dtype=np.float64)
    for crs in range(3):
        y = filter_axis(y, taps[crs], 2 - crs, intervals[crs])
    return y


def norm3(shape, taps, intervals):
    """N[s][r][c] = (W_c[c] * W_r[r]) * W_s[s]."""
    wc, wr, ws = (axis_weights(taps[k], shape[2 - k], intervals[k]) for k in range(3))
    return (wc[None, None, :] * wr[None, :, None]) * ws[:, None, None]


def map_filter(grid, taps, intervals, renormalize=False):
    """pdbeda_map_filter of a float32 grid: float32."""
    y = filter3(np.asarray(grid, dtype=np.float32), taps, intervals)
    if renormalize:
        n = norm3(y.shape, taps, intervals)
        ok = n > 0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            y = np.where(ok, y / np.where(ok, n, 1.0), 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return y.astype(np.float32)


def _clamp(x):
    return np.where(x < -1.0, -1.0, np.where(x > 1.0, 1.0, x))


def local_stats(a, b, taps, intervals, std_floor=0.0):
    """pdbeda_map_local_stats: a dict of float32 grids mean_a, std_a, z_a and, with b, mean_b, std_b, cc."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    n = norm3(a64.shape, taps, intervals)
    ok = n > 0
    safe = np.where(ok, n, 1.0)

    def moments(x):
        e = filter3(x, taps, intervals) / safe
        ee = filter3(x * x, taps, intervals) / safe
        t = ee - e * e
        v = np.where(t > 0, t, 0.0)
        s = np.sqrt(v)
        d = np.where(s > std_floor, s, std_floor)
        z = np.where(d > 0, (x - e) / np.where(d > 0, d, 1.0), 0.0)
        return e, v, s, z

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ea, va, sa, za = moments(a64)
        out = {"mean_a": ea, "std_a": sa, "z_a": za}
        if b is not None:
            b64 = np.asarray(b, dtype=np.float32).astype(np.float64)
            eb, vb, sb, _ = moments(b64)
            cov = filter3(a64 * b64, taps, intervals) / safe - ea * eb
            both = (va > 0) & (vb > 0)
            out.update(mean_b=eb, std_b=sb, cc=np.where(both, _clamp(cov / np.where(both, np.sqrt(va * vb), 1.0)), 0.0))
        return dict((k, np.where(ok, v, 0.0).astype(np.float32)) for k, v in out.items())
