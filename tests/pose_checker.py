"""The contract of pdbeda_pose_scores (include/pdbeda.h) restated in plain numpy: the yardstick of tests/test_gpu_pose.py, and the host plan of
pdb_eda_amd/csrc/pdbeda_poseplan.h restated for tests/test_pose_plan_host.py.  Nothing here comes from the product's native library.

Positions: p[i] = c[i] + fma(R[i][2], x[2], fma(R[i][0], x[0], R[i][1] * x[1])), the fused dot product restated as tests/resample_checker.py
restates it (``ccp4._fma`` element by element), the add unfused.  The grid position is resample_checker.xyz2frac (the device's, to the bit, on
skewed cells too).  The SAMPLE is qscore_checker.interp and is not restated: it is handed the grid position through a header in which a
coordinate IS its grid position (orthogonal, origin 0, step 1, axes in order -- (f - 0) / 1 is exact), with the map's own shape and wrap
intervals.  The score is a plain loop over the atoms, product and sum rounded separately.  No box, no staging: a result cannot depend on them.

The plan: the span of a centre's sphere along a crs axis is gradient_checker's arithmetic (the rule is pdbeda_gradplan.h's); the box, the
budget, the chunks and the carve are restated from pdbeda_poseplan.h."""
import math

import numpy as np

from pdb_eda_amd import ccp4

import gradient_checker
import qscore_checker
import resample_checker

MAX_ATOMS, MAX_ROTATIONS, MAX_TOP = 256, 2 ** 20, 64
LDS_BUDGET, GROW = 128 * 1024, 2
TABLE_BYTES, TABLE_ROW = 64 << 20, 13
OK, ATOMS, ROTATIONS, TOP, FLAG, COUNT, FRAG_VALUE, ROT_VALUE, CENTRE_VALUE, REACH, CENTRE_GRID = range(11)
ALLOW_OUTSIDE, GLOBAL_ONLY = 1, 2
_fma = np.frompyfunc(ccp4._fma, 3, 1)


# ---- the contract -----------------------------------------------------------------------------------------------------------------------------
def positions(frag, rot, centres):
    """(n_centres, n_rot, n_frag, 3): every atom of every pose."""
    x = np.asarray(frag, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    dot = np.empty((len(R), len(x), 3), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            p1 = R[:, None, i, 1] * x[None, :, 1]
            dot[:, :, i] = _fma(R[:, None, i, 2], x[None, :, 2], _fma(R[:, None, i, 0], x[None, :, 0], p1)).astype(np.float64)
        return c[:, None, None, :] + dot[None, :, :, :]


class _IndexSpace(object):
    """A header in which a coordinate is its own grid position; the shape and the wrap intervals are the map's."""

    def __init__(self, header):
        self.orthogonal, self.origin, self.gridLength, self.map2crs = True, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 1, 2]
        self.ncrs, self.crsInterval = header.ncrs, header.crsInterval


def sample(header, grid, xyz):
    """(values, valid) of pdbeda_interp_density at (n, 3) coordinates; NaN / False where that call would refuse the point."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = resample_checker.xyz2frac(header, np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
        sane = np.all(np.abs(f) < 2.0 ** 29, axis=1)      # (a NaN fails)
        v, ok, _ = qscore_checker.interp(_IndexSpace(header), np.asarray(grid, dtype=np.float32), np.where(sane[:, None], f, 0.0))
    return np.where(sane, v, np.nan), ok & sane


def scores(header, grid, frag, weights, rot, centres, floor=-np.inf, max_low=None, allow_outside=False):
    """dict ``scores`` (n_centres, n_rot) float64, ``low`` int32, ``kept`` bool, ``valid`` bool (every atom valid)."""
    p = positions(frag, rot, centres)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    v, ok = sample(header, grid, p.reshape(-1, 3))
    v, ok = v.reshape(p.shape[:3]), ok.reshape(p.shape[:3])
    s = np.zeros(p.shape[:2], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(len(w)):
            s = s + w[a] * v[:, :, a]
        low = (v < float(np.float32(floor))).sum(axis=2).astype(np.int32)
        s = np.where(np.isnan(s), np.nan, s)      # (the contract's one NaN)
    valid = ok.all(axis=2)
    limit = 2 ** 31 - 1 if max_low is None else int(max_low)
    kept = ~(low > limit) & ~np.isnan(s) & (valid | bool(allow_outside))
    return {"scores": s, "low": low, "kept": kept, "valid": valid}


def ranking(table, top_k):
    """(best_rot, best_score, best_low (n_centres, top_k), n_kept) of a ``scores`` table: score descending as numbers, then index ascending."""
    s, low, kept = table["scores"], table["low"], table["kept"]
    n = len(s)
    best_rot, best_score, best_low = np.full((n, top_k), -1, dtype=np.int32), np.zeros((n, top_k)), np.zeros((n, top_k), dtype=np.int32)
    for c in range(n):
        order = sorted(np.nonzero(kept[c])[0].tolist(), key=lambda r: (-float(s[c, r]), r))[:top_k]
        for k, r in enumerate(order):
            best_rot[c, k], best_score[c, k], best_low[c, k] = r, s[c, r], low[c, r]
    return best_rot, best_score, best_low, kept.sum(axis=1).astype(np.int32)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def radius_of(frag):
    x = np.asarray(frag, dtype=np.float64).reshape(-1, 3)
    return float(np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).max())


def check(n_frag, n_rot, n_centres, top_k, flags, frag, weights, rot, centres):
    """(refusal, offender, radius) of pose_check, in its order; the arrays as flat lists."""
    if n_frag < 1 or n_frag > MAX_ATOMS:
        return ATOMS, -1, 0.0
    if n_rot < 1 or n_rot > MAX_ROTATIONS:
        return ROTATIONS, -1, 0.0
    if top_k < 1 or top_k > MAX_TOP:
        return TOP, -1, 0.0
    if flags & ~(ALLOW_OUTSIDE | GLOBAL_ONLY):
        return FLAG, -1, 0.0
    if n_centres < 0 or n_centres >= 2 ** 31 or n_centres * n_rot >= 2 ** 31:
        return COUNT, -1, 0.0
    radius = 0.0
    for a in range(n_frag):
        x, y, z = frag[3 * a:3 * a + 3]
        if not all(math.isfinite(v) for v in (x, y, z, weights[a])):
            return FRAG_VALUE, a, radius
        radius = max(radius, math.sqrt((x * x + y * y) + z * z))
    for i, v in enumerate(rot):
        if not math.isfinite(v):
            return ROT_VALUE, i // 9, radius
    for i, v in enumerate(centres):
        if not math.isfinite(v):
            return CENTRE_VALUE, i // 3, radius
    return OK, -1, radius


def centre_ok(rows, off, c):
    return all(abs(((rows[k][0] * c[0] + rows[k][1] * c[1]) + rows[k][2] * c[2]) + off[k]) < float(2 ** 29) for k in range(3))


def lds_bytes(voxels):
    return 4 * voxels + 8 * ((voxels + 63) // 64)


def box(rows, off, norm, c, radius, global_only=False):
    """(lo [3], n [3], voxels or -1, staged) of pose_box."""
    lo, n, vox = [0] * 3, [0] * 3, 1
    for k in range(3):
        t0, t1, t2 = rows[k][0] * c[0], rows[k][1] * c[1], rows[k][2] * c[2]
        f = ((t0 + t1) + t2) + off[k]
        h = radius * norm[k]
        mag = (((abs(t0) + abs(t1)) + abs(t2)) + abs(off[k])) + (h + 1.0)
        w = h + gradient_checker.PAD * mag
        first, last = math.ceil(f - w), math.floor(f + w)
        lo[k], n[k] = int(first) - GROW, int(last - first) + 1 + 2 * GROW
        if n[k] > LDS_BUDGET // 4:
            vox = -1
        if vox >= 0:
            vox *= n[k]
    return lo, n, vox, int(not global_only and vox >= 0 and lds_bytes(vox) <= LDS_BUDGET)


def boxes(header, frag, centres, global_only=False):
    rows, off, norm, _ = gradient_checker.grid_of(header)
    r = radius_of(frag)
    return [box(rows, off, norm, [float(v) for v in c], r, global_only) for c in np.asarray(centres, dtype=np.float64).reshape(-1, 3)]


def counters(header, frag, centres, kept, global_only=False):
    """{"globalCentres", "maxStagedBox", "rejected"} of a call."""
    all_boxes = boxes(header, frag, centres, global_only)
    return {"globalCentres": sum(1 for b in all_boxes if not b[3]), "maxStagedBox": max([b[2] for b in all_boxes if b[3]] + [0]),
            "rejected": int(kept.size - kept.sum())}


def chunk(n_centres, n_rot):
    return max(1, min(n_centres, TABLE_BYTES // (TABLE_ROW * n_rot)))


def scratch_bytes(n_frag, n_rot, ch, top_k):
    """The carve of PoseScratch: every piece in whole 256-byte units."""
    up = lambda count, size: (count * size + 255) // 256 * 256
    return (up(3 * n_frag, 8) + up(n_frag, 8) + up(9 * n_rot, 8) + up(3 * ch, 8) + up(ch, 32) + up(ch * n_rot, 8) + up(ch * n_rot, 4) + up(ch * n_rot, 1)
            + up(ch * top_k, 4) + up(ch * top_k, 8) + up(ch * top_k, 4) + up(ch, 4))
