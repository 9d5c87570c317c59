"""The plain numpy restatement of pdbeda_map_resample (the contract: include/pdbeda.h).  Every step is the contract's unfused fp64 (numpy's
elementwise operations round once each); the two dot products of a skewed cell (crs2xyz, xyz2frac) are matvec3's,
fma(a2, v2, fma(a0, v0, a1 * v1)), through ``ccp4._fma`` -- so a grid position is the device's to the bit, and with it every floor, every
snap and every weight.  No tiles, no staging: a voxel is a row of arrays."""
import numpy as np

from pdb_eda_amd import ccp4

import qscore_checker

SNAP = 2.0 ** -26
_fma = np.frompyfunc(ccp4._fma, 3, 1)


def matvec3(mat, v):
    """pdbeda_device.h's matvec3 on (n, 3) rows."""
    m = np.asarray(mat, dtype=np.float64)
    out = np.empty((len(v), 3), dtype=np.float64)
    for i in range(3):
        p1 = m[i, 1] * v[:, 1]
        out[:, i] = _fma(m[i, 2], v[:, 2], _fma(m[i, 0], v[:, 0], p1)).astype(np.float64) if len(v) else 0.0
    return out


def all_crs(header):
    """Every stored voxel as (n, 3) integer crs triples, c fastest."""
    nc, nr, ns = (int(v) for v in header.ncrs)
    s, r, c = np.meshgrid(np.arange(ns), np.arange(nr), np.arange(nc), indexing="ij")
    return np.stack([c.ravel(), r.ravel(), s.ravel()], axis=1).astype(np.int64)


def crs2xyz(header, crs):
    """DensityHeader.crs2xyzCoord for integer crs, with the device's arithmetic."""
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    if header.orthogonal:
        return np.stack([crs[:, header.map2xyz[i]].astype(np.float64) * float(header.gridLength[i]) + float(header.origin[i]) for i in range(3)], axis=1)
    f = np.stack([(crs[:, header.map2xyz[i]] + int(header.crsStart[header.map2xyz[i]])).astype(np.float64) / float(header.xyzInterval[i]) for i in range(3)], axis=1)
    return matvec3(header.orthoMat, f)


def xyz2frac(header, xyz):
    """The fractional grid position in crs order, with the device's arithmetic (qscore_checker.frac with the fused dot product)."""
    if header.orthogonal:
        return qscore_checker.frac(header, xyz)
    fr = matvec3(header.deOrthoMat, xyz)
    q = np.stack([fr[:, i] * float(header.xyzInterval[i]) - float(header.crsStart[header.map2xyz[i]]) for i in range(3)], axis=1)
    return np.stack([q[:, header.map2crs[j]] for j in range(3)], axis=1)


def apply_operator(op, p):
    """x[i] = ((R[i][0] p[0] + R[i][1] p[1]) + R[i][2] p[2]) + t[i], unfused."""
    op = np.asarray(op, dtype=np.float64).reshape(3, 4)
    return np.stack([((op[i, 0] * p[:, 0] + op[i, 1] * p[:, 1]) + op[i, 2] * p[:, 2]) + op[i, 3] for i in range(3)], axis=1)


def snap(f):
    r = np.rint(f)
    return np.where(np.abs(f - r) <= SNAP, r, f)


def cubic_weights(t):
    """The four Catmull-Rom weights of the contract, in its operation order."""
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t]


def _fold(order, v, t):
    """One axis: v is the list of tap arrays (2 or 4), of which only the one at b counts where t == 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        if order == 1:
            return np.where(t == 0.0, v[0], v[0] + t * (v[1] - v[0]))
        w = cubic_weights(t)
        return np.where(t == 0.0, v[1], ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3])


def sample(header, grid, f, order):
    """(values as float64, valid) at snapped fractional positions f (n, 3)."""
    if order == 0:
        return qscore_checker.fetch(header, grid, np.rint(f).astype(np.int64))
    base = np.floor(f)
    t = f - base
    b = base.astype(np.int64)
    n_taps, k0 = (2, 0) if order == 1 else (4, 1)
    valid = np.ones(len(f), dtype=bool)
    ys = []
    for ks in range(n_taps):
        yr = []
        for kr in range(n_taps):
            v = []
            for kc in range(n_taps):
                value, ok = qscore_checker.fetch(header, grid, b + np.array([kc - k0, kr - k0, ks - k0]))
                used = ((t[:, 0] != 0.0) | (kc == k0)) & ((t[:, 1] != 0.0) | (kr == k0)) & ((t[:, 2] != 0.0) | (ks == k0))
                valid &= ok | ~used
                v.append(value)
            yr.append(_fold(order, v, t[:, 0]))
        ys.append(_fold(order, yr, t[:, 1]))
    return _fold(order, ys, t[:, 2]), valid


def positions(src_header, dst_header, op):
    """The snapped source grid positions of every destination voxel under one operator."""
    return snap(xyz2frac(src_header, apply_operator(op, crs2xyz(dst_header, all_crs(dst_header)))))


def resample(src_header, grid, dst_header, ops, order=1, mean=False, fill=0.0, base=None, alpha=1.0):
    """(out float32 [ns][nr][nc], count int [ns][nr][nc]) of pdbeda_map_resample."""
    ops = np.asarray(ops, dtype=np.float64).reshape(-1, 12)
    grid = np.asarray(grid, dtype=np.float32)
    p = crs2xyz(dst_header, all_crs(dst_header))
    n = len(p)
    count = np.zeros(n, dtype=np.int64)
    value = np.zeros(n, dtype=np.float64)
    for op in ops:
        f = snap(xyz2frac(src_header, apply_operator(op, p)))
        v, ok = sample(src_header, grid, f, order)
        if mean:
            with np.errstate(invalid="ignore", over="ignore"):
                value = np.where(ok, value + v, value)
            count += ok
        else:
            take = ok & (count == 0)
            value = np.where(take, v, value)
            count += take
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        val = value / np.maximum(count, 1).astype(np.float64) if mean else value
        res = (np.asarray(base, dtype=np.float32).reshape(-1).astype(np.float64) + float(alpha) * val) if base is not None else val
        out = np.where(count > 0, res.astype(np.float32), np.asarray(fill, dtype=np.float32))
    nc, nr, ns = (int(v) for v in dst_header.ncrs)
    out = out.astype(np.float32).reshape(ns, nr, nc)
    flat = out.reshape(-1).view(np.uint32)
    flat[count == 0] = np.asarray(fill, dtype=np.float32).reshape(1).view(np.uint32)[0]      # (the fill's bits, a NaN's payload included)
    return out, count.reshape(ns, nr, nc)


def same_bits(got, want):
    """Float32 arrays compared as uint32; where ``want`` is a NaN only the NaN-ness is compared."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
