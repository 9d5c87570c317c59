"""The contract of pdbeda_atom_moments (include/pdbeda.h) restated in plain numpy: the yardstick of tests/test_gpu_gradient.py, and the
host plan of pdb_eda_amd/csrc/pdbeda_gradplan.h restated for tests/test_gradient_plan_host.py.  Nothing here comes from the product's
native library.

``moments`` tests EVERY voxel of the domain against EVERY atom -- there is no box, so a box that fails to cover is caught --, forms the five
terms in fp64 exactly as the contract words them and sums each output with math.fsum: exact, then rounded once.

The bound of an output, |device - checker| <= N 2^-(S+1) + c 2^-52 sum|t|.
  N 2^-(S+1): each of the N terms of the output is rounded once to the quantum 2^-S, half a quantum at the most.
  c 2^-52 sum|t|: what the two sides may disagree on BEFORE that rounding, relative to each term.  dx, dy, dz and d2 are the same bits on
  both sides (IEEE products, sums and crs2xyzCoord).  The chain of a term t = (w * exp(-(k * d2))) * f, in units of 2^-52:
    the product k * d2 inside exp: half a unit of the argument, which exp amplifies by the argument itself, at most E_max = max k r^2 of
      the case -- 0.5 E_max per side, E_max in all (the product is the same IEEE operation on both sides; it is counted all the same);
    exp: one ulp on either side -- the device library and libm both promise that much --, 2 units;
    the product w * e: half a unit per side, 1 unit; the product by f: 1 unit (M0 has none: it is counted all the same);
    the conversion (double)sum on the device and the last rounding of fsum here: half a unit each of |output| <= sum|t|, 1 unit.
  c = 5 + E_max."""
import math

import numpy as np

MAX_TERMS = 6
PAD = 2.0 ** -30
OK, TERMS, FLAG, COUNT, XYZ, EXPO, RADIUS, REACH, BOX = range(9)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def grid_of(header, unique=False):
    """(rows [3][3], off [3], norm [3], dom [3]): the xyz -> crs map as pdbeda_atom_moments hands it to the plan."""
    rows, off = [[0.0] * 3 for _ in range(3)], [0.0] * 3
    for k in range(3):
        a = int(header.map2crs[k])
        if header.orthogonal:
            rows[k][a] = 1.0 / float(header.gridLength[a])
            off[k] = -(float(header.origin[a]) / float(header.gridLength[a]))
        else:
            for i in range(3):
                rows[k][i] = float(header.deOrthoMat[a][i]) * float(header.xyzInterval[a])
            off[k] = -float(header.crsStart[int(header.map2xyz[a])])
    dom = [int(v) for v in (header.uniqueNcrs if unique else header.ncrs)]
    dom = [min(d, int(n)) for d, n in zip(dom, header.ncrs)]
    return rows, off, norms(rows), dom


def norms(rows):
    return [math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) for r in rows]


def check(n_atoms, n_terms, flags, xyz, expo, radii):
    """(refusal, atom, r_top) of grad_check, in its order."""
    if n_terms < 1 or n_terms > MAX_TERMS:
        return TERMS, -1, 0.0
    if flags & ~1:
        return FLAG, -1, 0.0
    if n_atoms < 0 or n_atoms >= 2 ** 31:
        return COUNT, -1, 0.0
    for i, v in enumerate(xyz):
        if not math.isfinite(v):
            return XYZ, i // 3, 0.0
    for i, v in enumerate(expo):
        if not math.isfinite(v) or v < 0:
            return EXPO, i // n_terms, 0.0
    top = 0.0
    for i, v in enumerate(radii):
        v = float(np.float32(v))
        if not math.isfinite(v) or not v > 0:
            return RADIUS, i, top
        top = max(top, v)
    return OK, -1, top


def reach_ok(norm, r_max):
    return all(r_max * n < float(2 ** 29) for n in norm)


def box(rows, off, norm, dom, xyz, radius):
    """(lo [3], n [3], voxels, clipped) of grad_box."""
    lo, hi, empty, clipped = [0.0] * 3, [0.0] * 3, False, False
    for k in range(3):
        t0, t1, t2 = rows[k][0] * xyz[0], rows[k][1] * xyz[1], rows[k][2] * xyz[2]
        f = ((t0 + t1) + t2) + off[k]
        h = radius * norm[k]
        mag = (((abs(t0) + abs(t1)) + abs(t2)) + abs(off[k])) + (h + 1.0)
        w = h + PAD * mag
        if not math.isfinite(f) or not math.isfinite(w):
            empty = clipped = True
            continue
        first, last, top = math.ceil(f - w), math.floor(f + w), dom[k] - 1
        if first < 0 or last > top:
            clipped = True
        lo[k], hi[k] = max(first, 0), min(last, top)
        if not lo[k] <= hi[k]:
            empty = True
    if empty:
        return [0, 0, 0], [0, 0, 0], 0, clipped
    n = [int(hi[k] - lo[k]) + 1 for k in range(3)]
    return [int(v) for v in lo], n, n[0] * n[1] * n[2], clipped


def quantum_shift(bound):
    s = 40
    if bound > 0.0 and math.isfinite(bound):
        s = 61 - math.frexp(bound)[1]
    return max(-900, min(s, 900))


def shift(max_abs_w, r_max, v_max):
    return quantum_shift((max_abs_w * max(1.0, r_max * r_max)) * float(max(v_max, 2 ** 22)))


def plan(header, xyz, radii, max_abs_w, unique=False):
    """(S, V_max, clipped atoms, boxes) for a call the checks accept."""
    rows, off, norm, dom = grid_of(header, unique)
    rad = np.asarray(radii, dtype=np.float32).astype(np.float64)
    boxes = [box(rows, off, norm, dom, [float(v) for v in p], float(r)) for p, r in zip(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), rad)]
    v_max = max([b[2] for b in boxes] + [0])
    return shift(float(max_abs_w), float(rad.max()) if len(rad) else 0.0, v_max), v_max, sum(1 for b in boxes if b[3]), boxes


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------------
def domain_crs(header, unique=False):
    nc, nr, ns = (int(v) for v in (header.uniqueNcrs if unique else header.ncrs))
    nc, nr, ns = min(nc, int(header.ncrs[0])), min(nr, int(header.ncrs[1])), min(ns, int(header.ncrs[2]))
    s, r, c = np.meshgrid(np.arange(ns), np.arange(nr), np.arange(nc), indexing="ij")
    return np.stack([c.reshape(-1), r.reshape(-1), s.reshape(-1)], axis=1).astype(np.int32)


_where = {}


def voxel_xyz(header, crs, key=None, crs2xyz=None):
    """The voxels' coordinates from the header's crs2xyzCoord, or from a callable the caller hands in (on a skewed cell, whose host np.dot is not
    pinned to the bit, the GPU test hands in the device's crs2xyz, which tests/test_gpu_voxel.py pins)."""
    if key is not None and key in _where:
        return _where[key]
    if crs2xyz is not None:
        out = np.asarray(crs2xyz(crs), dtype=np.float64).reshape(-1, 3)
    else:
        out = np.array([header.crs2xyzCoord([int(v) for v in one]) for one in crs], dtype=np.float64).reshape(-1, 3)
    if key is not None:
        _where[key] = out
    return out


def moments(header, weight, xyz, expo, radii, unique=False, key=None, crs2xyz=None):
    """dict: ``exact`` and ``abs`` ((n, terms, 5): the fsum of the terms and of their magnitudes), ``nVoxels`` (n,), ``e_max``,
    ``nearest_sphere`` (min |sqrt(d2) - radius| over all pairs, exact hits excluded) and ``on_sphere`` (the number of exact hits).
    ``key``: a name under which the voxel coordinates of this header and domain are kept for the next call."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    expo = np.asarray(expo, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, 1))
    rad = np.asarray(radii, dtype=np.float32).astype(np.float64).reshape(-1)
    crs = domain_crs(header, unique)
    where = voxel_xyz(header, crs, None if key is None else (key, unique, crs2xyz is not None), crs2xyz)
    w_all = np.asarray(weight)
    if w_all.dtype != np.float64:                                       # (the device's map is float32; a float64 array -- the host tests' residuals -- is taken as it is)
        w_all = w_all.astype(np.float32)
    w_all = w_all.reshape(int(header.ncrs[2]), int(header.ncrs[1]), int(header.ncrs[0]))
    w = w_all[crs[:, 2], crs[:, 1], crs[:, 0]].astype(np.float64)
    nt = expo.shape[1]
    exact, mags, count = np.zeros((n, nt, 5)), np.zeros((n, nt, 5)), np.zeros(n, dtype=np.int32)
    nearest, hits, e_max = np.inf, 0, 0.0
    for a in range(n):
        dx, dy, dz = where[:, 0] - xyz[a, 0], where[:, 1] - xyz[a, 1], where[:, 2] - xyz[a, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d = np.sqrt(d2)
        inside = d <= rad[a]
        hit = d == rad[a]
        hits += int(hit.sum())
        gap = np.abs(d - rad[a])[~hit]
        if gap.size:
            nearest = min(nearest, float(gap.min()))
        count[a] = int(inside.sum())
        dx, dy, dz, d2, wa = dx[inside], dy[inside], dz[inside], d2[inside], w[inside]
        for j in range(nt):
            if d2.size:
                e_max = max(e_max, float((expo[a, j] * d2).max()))
            t0 = wa * np.exp(-(expo[a, j] * d2))
            for q, t in enumerate((t0, t0 * dx, t0 * dy, t0 * dz, t0 * d2)):
                exact[a, j, q] = math.fsum(t.tolist())
                mags[a, j, q] = math.fsum(np.abs(t).tolist())
    return {"exact": exact, "abs": mags, "nVoxels": count, "e_max": e_max, "nearest_sphere": nearest, "on_sphere": hits}


def bounds(got, shift_s):
    """The bound of every output of ``moments`` at the shift S (the derivation: this module's docstring)."""
    c = 5.0 + got["e_max"]
    return got["nVoxels"].astype(np.float64)[:, None, None] * 2.0 ** -(shift_s + 1) + c * 2.0 ** -52 * got["abs"]
