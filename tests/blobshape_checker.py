"""A plain numpy restatement of the contract of pdbeda_bloblist_moments (include/pdbeda.h) and of the shape columns that
pdb_eda_amd.ccp4.blobShapeFinish derives from it.  Integer columns are exact (Python integers), weighted sums are fp64
(math.fsum: the exact sum, rounded once), and the Angstrom quantities are computed THE DIRECT WAY -- from the xyz of every voxel
(header.crs2xyz_array) and covariance sums over them -- not through M C M^T as the product does: two roads to the same numbers."""
import math

import numpy as np

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def point_density(header, grid, crs):
    """utils.getPointDensityFromCrs for an (n, 3) array of raw crs: periodic wrap, 0 where nothing is stored (float64 of the float32)."""
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    idx, ok = [], np.ones(len(crs), dtype=bool)
    for k in range(3):
        n, interval = int(header.ncrs[k]), int(header.crsInterval[k])
        v = crs[:, k].copy()
        out = (v < 0) | (v >= n)
        v[out] = np.mod(v[out], interval)                # (numpy's mod is Python's floor mod)
        ok &= ~((v >= n) & (v < interval)) & (v >= 0)
        idx.append(np.clip(v, 0, n - 1))
    rho = np.asarray(grid)[idx[2], idx[1], idx[0]].astype(np.float64)
    rho[~ok] = 0.0
    return rho


def _fsum_columns(a):
    return [math.fsum(a[:, k].tolist()) for k in range(a.shape[1])]


def _principal_lengths(cov):
    return np.sqrt(np.maximum(np.linalg.eigvalsh(cov)[::-1], 0.0))


def shape(header, grid, crs, offsets, whole_map=False):
    """Every column, one row per blob; crs (N, 3) raw voxels grouped by blob, offsets (blobs + 1)."""
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    nb = len(offsets) - 1
    rho_all = point_density(header, grid, crs)
    xyz_all = header.crs2xyz_array(crs) if len(crs) else np.zeros((0, 3))
    step = header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3)))          # row k: the xyz step of crs axis k
    unique = [int(v) for v in header.uniqueNcrs]
    out = {"n": np.zeros(nb, np.int64), "boxLo": np.zeros((nb, 3), np.int32), "boxHi": np.zeros((nb, 3), np.int32), "extremeCrs": np.zeros((nb, 3), np.int32),
           "extreme": np.zeros(nb, np.float32), "s1": [], "s2": [], "sw": np.zeros(nb), "sw1": np.zeros((nb, 3)), "sw2": np.zeros((nb, 6)),
           "boxExtent": np.zeros((nb, 3)), "boxDiagonal": np.zeros(nb), "onBorder": np.zeros(nb, bool), "extremeXyz": np.zeros((nb, 3)),
           "weightedCentroid": np.zeros((nb, 3)), "secondMomentXyz": np.zeros((nb, 3, 3)), "weightedSecondMomentXyz": np.zeros((nb, 3, 3)),
           "principalLengths": np.zeros((nb, 3)), "weightedPrincipalLengths": np.zeros((nb, 3)), "anisotropy": np.zeros(nb)}
    for b in range(nb):
        v, rho, xyz = crs[offsets[b]:offsets[b + 1]], rho_all[offsets[b]:offsets[b + 1]], xyz_all[offsets[b]:offsets[b + 1]]
        n = len(v)
        lo, hi = v.min(axis=0), v.max(axis=0)
        w = np.abs(rho)
        tied = np.nonzero(w == w.max())[0]
        first = tied[np.lexsort((v[tied, 2], v[tied, 1], v[tied, 0]))[0]]          # first in (c, r, s) order, c most significant
        d = v - lo
        assert n * int(d.max(initial=0)) ** 2 < 2 ** 62                            # (the int64 sums below are exact)
        dd = np.stack([d[:, i] * d[:, j] for i, j in PAIRS], axis=1)
        out["n"][b] = n
        out["boxLo"][b], out["boxHi"][b], out["extremeCrs"][b], out["extreme"][b] = lo, hi, v[first], rho[first]
        out["s1"].append([int(x) for x in d.sum(axis=0)])
        out["s2"].append([int(x) for x in dd.sum(axis=0)])
        out["sw"][b] = math.fsum(w.tolist())
        out["sw1"][b] = _fsum_columns(w[:, None] * d)
        out["sw2"][b] = _fsum_columns(w[:, None] * dd)
        # Angstrom quantities, straight from the voxels' xyz
        width = (hi - lo + 1).astype(np.float64)
        out["boxExtent"][b] = width * np.linalg.norm(step, axis=1)
        out["boxDiagonal"][b] = np.linalg.norm(width.dot(step))
        out["onBorder"][b] = whole_map and any(lo[k] <= 0 or hi[k] >= unique[k] - 1 for k in range(3))
        out["extremeXyz"][b] = xyz[first]
        centre = xyz.mean(axis=0)
        cov = (xyz - centre).T.dot(xyz - centre) / n
        out["secondMomentXyz"][b] = cov
        out["principalLengths"][b] = _principal_lengths(cov)
        l1, l3 = out["principalLengths"][b][0], out["principalLengths"][b][2]
        out["anisotropy"][b] = 1.0 - l3 / l1 if l1 > 0 else 0.0
        total = w.sum()
        if total > 0:
            wc = (w[:, None] * xyz).sum(axis=0) / total
            wcov = ((xyz - wc) * w[:, None]).T.dot(xyz - wc) / total
            out["weightedCentroid"][b], out["weightedSecondMomentXyz"][b], out["weightedPrincipalLengths"][b] = wc, wcov, _principal_lengths(wcov)
        else:
            out["weightedCentroid"][b], out["weightedSecondMomentXyz"][b], out["weightedPrincipalLengths"][b] = np.nan, np.nan, np.nan
    out["s1"] = np.array(out["s1"], dtype=np.int64).reshape(nb, 3)
    out["s2"] = np.array(out["s2"], dtype=np.int64).reshape(nb, 6)
    return out


def anisotropy_bound(want, tol):
    """What an error of ``tol`` (A^2) in the principal variances can move 1 - l3 / l1 by, per blob, from the checker's lengths:
    |sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)), so l3 moves by at most min(sqrt(tol), tol / l3) and l1 by tol / l1;
    l3' / l1' - l3 / l1 = dl3 / l1' + l3 dl1 / (l1 l1') and l3 <= l1, l1' >= l1 / 2 (tol is far below l1^2 for a blob of two voxels or
    more), which gives 2 (dl3 + dl1) / l1.  A flat or thin blob gets sqrt(tol) / l1, a full one about tol / l1^2.  (1e-15: the roundings of the quotient.)"""
    l1, l3 = want["principalLengths"][:, 0], want["principalLengths"][:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        dl3 = np.minimum(np.sqrt(tol), np.where(l3 > 0, tol / l3, np.inf))
        return np.where(l1 > 0, 2.0 * (dl3 + tol / l1) / l1, 0.0) + 1e-15
