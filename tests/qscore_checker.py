"""The plain numpy restatement of pdbeda_interp_density and pdbeda_atom_qscores (the contracts: include/pdbeda.h).  No cell grid: a
sample point is tested against EVERY atom; the correlation is the two-pass Pearson over the explicit list of kept points.

Sample points and squared distances are evaluated in the contract's unfused fp64 (numpy's elementwise operations round once each),
so every accept / reject decision -- shell_n, n_points -- is the device's to the bit.  The fractional grid position is exact
for orthogonal cells; for skewed cells the dot product is not the device's fused one, so a position may differ in its last bits:
that moves an interpolated value by nothing that matters, and a ``valid`` flag only for a point on a face of a voxel
(``near_integer`` reports how close any point came)."""
import numpy as np


def frac(header, xyz):
    """(n, 3) coordinates -> (n, 3) fractional grid positions in crs order: xyz2crsCoord without its round()."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    q = np.empty_like(xyz)
    if header.orthogonal:
        for i in range(3):
            q[:, i] = (xyz[:, i] - float(header.origin[i])) / float(header.gridLength[i])
    else:
        m = np.asarray(header.deOrthoMat, dtype=np.float64)
        for i in range(3):
            fr = (m[i, 1] * xyz[:, 1] + m[i, 0] * xyz[:, 0]) + m[i, 2] * xyz[:, 2]
            q[:, i] = fr * float(header.xyzInterval[i]) - float(header.crsStart[header.map2xyz[i]])
    return np.stack([q[:, header.map2crs[j]] for j in range(3)], axis=1)


def _wrap(v, n, interval):
    """utils.getPointDensityFromCrs's rule along one axis: (wrapped index, stored)."""
    w = np.where((v < 0) | (v >= n), np.mod(v, interval), v)
    return w, ~((w >= n) & (w < interval))


def fetch(header, grid, crs):
    """(values as float64 -- 0 where nothing is stored --, stored) of integer crs triples."""
    idx, ok = [], np.ones(len(crs), dtype=bool)
    for k in range(3):
        w, good = _wrap(crs[:, k], int(header.ncrs[k]), int(header.crsInterval[k]))
        idx.append(np.where(good, w, 0))
        ok &= good
    values = grid[idx[2], idx[1], idx[0]].astype(np.float64)
    return np.where(ok, values, 0.0), ok


def interp(header, grid, xyz):
    """(values, valid, f): the trilinear interpolant of pdbeda_interp_density at (n, 3) coordinates."""
    f = frac(header, xyz)
    base = np.floor(f)
    t = f - base
    b = base.astype(np.int64)
    v, valid = [], np.ones(len(f), dtype=bool)
    for k in range(8):
        value, ok = fetch(header, grid, b + np.array([k & 1, (k >> 1) & 1, k >> 2]))
        v.append(value)
        valid &= ok
    lerp = lambda a, c, w: a + w * (c - a)
    c00, c10, c01, c11 = lerp(v[0], v[1], t[:, 0]), lerp(v[2], v[3], t[:, 0]), lerp(v[4], v[5], t[:, 0]), lerp(v[6], v[7], t[:, 0])
    return lerp(lerp(c00, c10, t[:, 1]), lerp(c01, c11, t[:, 1]), t[:, 2]), valid, f


def _d2(p, b):
    d = p - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def accepted(xyz, atom, radii, unit):
    """[shell][candidate] -> (points, kept): the sample points of atom ``atom`` on the shells ``radii`` and whether NO other atom (by
    index) is strictly nearer to them than the atom itself."""
    a = xyz[atom]
    points = a + radii[:, None, None] * unit[None, :, :]
    own = _d2(points, a)
    nearer = np.zeros(own.shape, dtype=bool)
    others = np.delete(xyz, atom, axis=0)
    for lo in range(0, len(others), 128):          # (in slices only to bound the memory of the [shell][candidate][atom] table)
        b = others[lo:lo + 128]
        dx, dy, dz = (points[:, :, k, None] - b[None, None, :, k] for k in range(3))
        nearer |= (((dx * dx + dy * dy) + dz * dz) < own[:, :, None]).any(axis=2)
    return points, ~nearer


def pearson(x, y):
    """Two passes; NaN for fewer than two points, a flat or a non-finite x, a flat y; clipped to [-1, 1]."""
    if len(x) < 2 or not np.all(np.isfinite(x)) or x.min() == x.max() or y.min() == y.max():
        return float("nan")
    dx, dy = x - x.mean(), y - y.mean()
    return float(np.clip((dx * dy).sum() / (np.sqrt((dx * dx).sum()) * np.sqrt((dy * dy).sum())), -1.0, 1.0))


def qscores(header, grid, xyz, scored, step, ref, unit, offsets, min_points):
    """pdbeda_atom_qscores.  Besides the contract's outputs: ``ratio`` (variance / mean square of an atom's sampled values: the
    conditioning of its correlation; NaN without a finite q), ``near_integer`` (the smallest distance of a kept point's grid
    position from an integer) and ``neighbours`` (atoms with another index within 2 R_max (1 + 1e-6))."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    scored = np.arange(len(xyz)) if scored is None else np.asarray(scored, dtype=np.int64)
    ref, unit, offsets = np.asarray(ref, dtype=np.float64), np.asarray(unit, dtype=np.float64).reshape(-1, 3), [int(v) for v in offsets]
    shells, levels = len(ref), len(offsets) - 1
    radii = np.arange(shells, dtype=np.float64) * float(np.float32(step))
    reach = 2.0 * radii[-1] * (1.0 + 1e-6)
    out = {"q": np.full(len(scored), np.nan), "n_points": np.zeros(len(scored), np.int32), "shell_n": np.zeros((len(scored), shells), np.int32),
           "shell_mean": np.zeros((len(scored), shells)), "valid": np.zeros(len(scored), bool), "ratio": np.full(len(scored), np.nan),
           "neighbours": np.zeros(len(scored), np.int64), "near_integer": np.inf}
    for row, atom in enumerate(scored.tolist()):
        # level by level, only the shells that have not stopped yet (a candidate is tested against every atom all the same)
        chosen, open_shells = {}, np.arange(1, shells)
        for l in range(levels):
            if len(open_shells) == 0:
                break
            points, keep = accepted(xyz, atom, radii[open_shells], unit[offsets[l]:offsets[l + 1]])
            still = []
            for j, k in enumerate(open_shells.tolist()):
                if keep[j].sum() >= min_points or l == levels - 1:
                    chosen[k] = points[j, keep[j]]
                else:
                    still.append(k)
            open_shells = np.array(still, dtype=np.int64)
        kept_points = np.concatenate([xyz[atom][None, :]] + [chosen[k] for k in range(1, shells)])
        kept_shell = np.concatenate([np.zeros(1, dtype=np.int64)] + [np.full(len(chosen[k]), k, dtype=np.int64) for k in range(1, shells)])
        values, ok, f = interp(header, grid, kept_points)
        out["near_integer"] = min(out["near_integer"], float(np.abs(f - np.rint(f)).min()))
        counts = np.bincount(kept_shell, minlength=shells)
        out["shell_n"][row] = counts
        out["n_points"][row] = len(values)
        out["valid"][row] = bool(ok.all())
        for k in np.nonzero(counts)[0]:
            out["shell_mean"][row, k] = values[kept_shell == k].mean()
        q = pearson(values, ref[kept_shell]) if (counts > 0).sum() >= 2 else float("nan")
        out["q"][row] = q
        if q == q:
            out["ratio"][row] = values.var() / (values * values).mean()
        near = _d2(xyz[atom], xyz) <= reach * reach
        out["neighbours"][row] = int(near.sum()) - int(near[atom])
    return out
