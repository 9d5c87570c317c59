"""The model-density and pair-moment contracts of include/pdbeda.h (pdbeda_model_density, pdbeda_map_pair_moments) restated in plain
numpy: the yardstick of tests/test_gpu_model.py.  Nothing here comes from the product's native library: brute force over all STORED
voxels x all atoms (in chunks), d2 = (dx*dx + dy*dy) + dz*dz in fp64, np.sqrt(d2) <= float32(radius), a term amp * np.exp(-(expo * d2)),
and the value of a voxel is math.fsum of its terms: exact, then rounded once.  The voxel coordinates come from the header's crs2xyzCoord or
from a callable the caller hands in."""
import math

import numpy as np


def stored_crs(header):
    """Every stored voxel as (n x 3) int32 crs triples, c fastest."""
    nc, nr, ns = (int(v) for v in header.ncrs)
    s, r, c = np.meshgrid(np.arange(ns), np.arange(nr), np.arange(nc), indexing="ij")
    return np.stack([c.reshape(-1), r.reshape(-1), s.reshape(-1)], axis=1).astype(np.int32)


def voxel_xyz(header, crs, crs2xyz=None):
    if crs2xyz is None:
        return np.array([header.crs2xyzCoord([int(v) for v in one]) for one in crs], dtype=np.float64).reshape(-1, 3)
    return np.asarray(crs2xyz(crs), dtype=np.float64).reshape(-1, 3)


def shift_rule(n_gridded, a_max):
    """S: the largest integer <= 40 with n_gridded * a_max * 2^S <= 2^62 (fp64); 40 when the product is 0."""
    prod = float(n_gridded) * float(a_max)
    s = 40
    if not prod > 0.0:
        return s
    while math.ldexp(prod, s) > 2.0 ** 62:
        s -= 1
    return s


def a_max(amp):
    amp = np.asarray(amp, dtype=np.float64)
    if amp.size == 0:
        return 0.0
    total = np.zeros(len(amp))
    for j in range(amp.shape[1]):          # (index order, as the host adds them)
        total = total + np.abs(amp[:, j])
    return float(total.max())


def terms_2d(amp, n_atoms):
    amp = np.asarray(amp, dtype=np.float64)
    return amp.reshape(n_atoms, -1) if n_atoms else np.zeros((0, 1))


def density(header, xyz, amp, expo, radii, crs2xyz=None, chunk=1024):
    """dict over the stored voxels ([ns][nr][nc]): ``exact`` (float64, the fsum of the voxel's terms), ``count`` (atoms that contribute),
    ``on_sphere`` (some pair has sqrt(d2) == radius), and over all pairs ``nearest_sphere`` (min |sqrt(d2) - radius|, excluding exact
    hits) and ``smallest_term`` (min |term| over the contributing pairs with a non-zero amplitude)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n_atoms = len(xyz)
    amp, expo = terms_2d(amp, n_atoms), terms_2d(expo, n_atoms)
    rad = np.asarray(radii, dtype=np.float32).astype(np.float64).reshape(-1)
    crs = stored_crs(header)
    where = voxel_xyz(header, crs, crs2xyz)
    n_vox = len(crs)
    exact, count, on_sphere = np.zeros(n_vox), np.zeros(n_vox, dtype=np.int64), np.zeros(n_vox, dtype=bool)
    nearest, smallest = np.inf, np.inf
    for a in range(0, n_vox if n_atoms else 0, chunk):
        p = where[a:a + chunk]
        dx, dy, dz = p[:, None, 0] - xyz[None, :, 0], p[:, None, 1] - xyz[None, :, 1], p[:, None, 2] - xyz[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d = np.sqrt(d2)
        inside = d <= rad[None, :]
        hit = d == rad[None, :]
        gap = np.abs(d - rad[None, :])[~hit]
        if gap.size:
            nearest = min(nearest, float(gap.min()))
        count[a:a + chunk] = inside.sum(axis=1)
        on_sphere[a:a + chunk] = hit.any(axis=1)
        terms = [amp[None, :, j] * np.exp(-(expo[None, :, j] * d2)) for j in range(amp.shape[1])]
        for k in np.nonzero(inside.any(axis=1))[0]:
            mine = np.concatenate([t[k][inside[k]] for t in terms])
            exact[a + k] = math.fsum(mine.tolist())
            live = np.abs(mine[mine != 0.0])
            if live.size:
                smallest = min(smallest, float(live.min()))
    shape = (int(header.ncrs[2]), int(header.ncrs[1]), int(header.ncrs[0]))
    return {"exact": exact.reshape(shape), "count": count.reshape(shape), "on_sphere": on_sphere.reshape(shape), "nearest_sphere": nearest,
            "smallest_term": smallest}


def pair_moments(header, a, b, floor=None):
    """(n, [Sa, Sb, Saa, Sbb, Sab], the same five sums over the absolute terms) over the voxels of the non-repeating box where both maps are
    finite and b > float32(floor) (strict; None: every finite pair); products in fp64, sums by math.fsum."""
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    shape = (int(header.ncrs[2]), int(header.ncrs[1]), int(header.ncrs[0]))
    x = np.asarray(a, dtype=np.float32).reshape(shape)[:us, :ur, :uc].astype(np.float64).reshape(-1)
    y = np.asarray(b, dtype=np.float32).reshape(shape)[:us, :ur, :uc].astype(np.float64).reshape(-1)
    keep = np.isfinite(x) & np.isfinite(y)
    if floor is not None:
        keep &= y > float(np.float32(floor))
    x, y = x[keep], y[keep]
    cols = [x, y, x * x, y * y, x * y]
    return int(keep.sum()), np.array([math.fsum(c.tolist()) for c in cols]), np.array([math.fsum(np.abs(c).tolist()) for c in cols])


def correlation(n, sums):
    """(cc, scale, offset) of a ~ scale * b + offset from the pair moments; NaN where a variance is zero."""
    sa, sb, saa, sbb, sab = (float(v) for v in sums)
    if n == 0:
        return float("nan"), float("nan"), float("nan")
    va, vb, cov = saa - sa * sa / n, sbb - sb * sb / n, sab - sa * sb / n
    cc = cov / math.sqrt(va * vb) if va > 0 and vb > 0 else float("nan")
    scale = cov / vb if vb > 0 else float("nan")
    return cc, scale, (sa - scale * sb) / n if vb > 0 else float("nan")


def truncated_fraction(n_sigma):
    """The share of a 3-D Gaussian's integral that lies beyond n_sigma standard deviations: erfc(n / sqrt 2) + sqrt(2 / pi) n exp(-n^2 / 2)."""
    n = float(n_sigma)
    return math.erfc(n / math.sqrt(2.0)) + math.sqrt(2.0 / math.pi) * n * math.exp(-0.5 * n * n)
