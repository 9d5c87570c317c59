"""Plain numpy restatement of the peak-search contract (include/pdbeda.h, pdbeda_map_peaks) -- the yardstick of the peak tests.
It shares no code with the library: 26 shifted views of the unique box padded with "no neighbour", the total order on voxels,
one parabola per axis in fp64, ``header.crs2xyz_array`` on the fractional crs."""
import itertools

import numpy as np


def find_peaks(header, grid, cutoff):
    """grid: float32 [ns][nr][nc] as stored.  Returns a dict of arrays in list order (descending |height|, ties by c-major
    position): crs (n x 3 int32, raw), height (float32), on_border (bool), offset (n x 3), refined_height, refined_xyz,
    key (c-major position)."""
    t = np.float32(cutoff)
    assert t != 0
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    box = np.ascontiguousarray(np.asarray(grid, dtype=np.float32)[:us, :ur, :uc])      # the domain of createFullCrsList
    D = np.transpose(box, (2, 1, 0))                                                  # D[c, r, s]
    sign = 1 if t > 0 else -1
    with np.errstate(invalid="ignore"):
        peak = (D >= t) if sign > 0 else (D <= t)                                      # inclusive; NaN fails
        pad = np.zeros((uc + 2, ur + 2, us + 2), dtype=np.float32)
        pad[1:-1, 1:-1, 1:-1] = D
        inside = np.zeros(pad.shape, dtype=bool)                                       # False = "no neighbour"
        inside[1:-1, 1:-1, 1:-1] = True
        n_neighbours = np.zeros(D.shape, dtype=np.int32)
        for dc, dr, ds in itertools.product((-1, 0, 1), repeat=3):
            if (dc, dr, ds) == (0, 0, 0):
                continue
            view = (slice(1 + dc, 1 + dc + uc), slice(1 + dr, 1 + dr + ur), slice(1 + ds, 1 + ds + us))
            nb, has = pad[view], inside[view]
            first = (dc, dr, ds) > (0, 0, 0)                  # the voxel comes first in c-major order: the neighbour is later
            beats = (D > nb) if sign > 0 else (D < nb)
            if first:
                beats = beats | (D == nb)
            peak &= beats | ~has
            n_neighbours += has
    crs = np.stack(np.nonzero(peak), axis=1).astype(np.int32)
    height = D[peak]
    key = (crs[:, 0].astype(np.int64) * ur + crs[:, 1]) * us + crs[:, 2]
    order = np.lexsort((key, -np.abs(height.astype(np.float64))))
    crs, height, key = crs[order], height[order], key[order]
    on_border = n_neighbours[peak][order] < 26
    v = height.astype(np.float64)
    dims = (uc, ur, us)
    offset = np.zeros((len(crs), 3), dtype=np.float64)
    terms = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for axis in range(3):
            x = crs[:, axis]
            both = (x > 0) & (x + 1 < dims[axis])
            lo_at, hi_at = crs.copy(), crs.copy()
            lo_at[:, axis] = np.where(both, x - 1, x)
            hi_at[:, axis] = np.where(both, x + 1, x)
            a = D[lo_at[:, 0], lo_at[:, 1], lo_at[:, 2]].astype(np.float64)
            b = D[hi_at[:, 0], hi_at[:, 1], hi_at[:, 2]].astype(np.float64)
            den = (a - 2.0 * v) + b
            use = both & (den != 0)
            off = np.where(use, (0.5 * (a - b)) / np.where(use, den, 1.0), 0.0)
            off = np.where(off < -0.5, -0.5, np.where(off > 0.5, 0.5, off))
            offset[:, axis] = off
            terms.append(np.where(use, (a - b) * off, 0.0))
    total = (terms[0] + terms[1]) + terms[2]
    refined_height = v - 0.25 * total
    refined_xyz = header.crs2xyz_array(crs.astype(np.float64) + offset) if len(crs) else np.zeros((0, 3))
    return {"crs": crs, "height": height, "on_border": on_border, "offset": offset, "refined_height": refined_height,
            "refined_xyz": refined_xyz, "key": key}
