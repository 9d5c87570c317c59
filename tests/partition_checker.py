"""The nearest-atom partition contract of include/pdbeda.h (pdbeda_map_partition) restated in plain numpy: the yardstick of
tests/test_gpu_partition.py.  Nothing here comes from the product's native library: brute force over all voxels of the
non-repeating box x all atoms (in chunks), d2 = (dx*dx + dy*dy) + dz*dz in fp64, np.argmin (the FIRST of equal minima: the
lowest atom index), np.sqrt(d2) <= float32(max_distance), and the sums are math.fsum (exact, then rounded once) over the finite voxels.  The voxel
coordinates come from the header's crs2xyzCoord or from a callable the caller hands in."""
import math

import numpy as np


def box_crs(header):
    """The voxels of the non-repeating box as (n x 3) int32 crs triples, c fastest."""
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    s, r, c = np.meshgrid(np.arange(us), np.arange(ur), np.arange(uc), indexing="ij")
    return np.stack([c.reshape(-1), r.reshape(-1), s.reshape(-1)], axis=1).astype(np.int32)


def box_grid(header, grid):
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    return np.asarray(grid, dtype=np.float32).reshape(header.ncrs[2], header.ncrs[1], header.ncrs[0])[:us, :ur, :uc]


def partition(header, grid, xyz, max_distance, cutoff, crs2xyz=None, chunk=4096):
    """dict: owner ((us, ur, uc) int32, -1 = unowned), per atom n / sum / n_pos / sum_pos / n_neg / sum_neg, unowned_n (3,),
    unowned_sum (4,: sum, sum_pos, sum_neg, sum_sq), and two diagnostics over the voxels: tied (two or more atoms at the minimum d2,
    the minimum within the distance) and on_sphere (the owner's distance is exactly max_distance)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    rho = box_grid(header, grid).astype(np.float64).reshape(-1)
    crs = box_crs(header)
    if crs2xyz is None:
        where = np.array([header.crs2xyzCoord([int(v) for v in one]) for one in crs], dtype=np.float64).reshape(-1, 3)
    else:
        where = np.asarray(crs2xyz(crs), dtype=np.float64).reshape(-1, 3)
    maxd, cut = float(np.float32(max_distance)), float(np.float32(cutoff))
    n_vox, n_atoms = len(crs), len(xyz)
    owner = np.full(n_vox, -1, dtype=np.int32)
    tied, on_sphere = np.zeros(n_vox, dtype=bool), np.zeros(n_vox, dtype=bool)
    for a in range(0, n_vox, chunk if n_atoms else n_vox):
        p = where[a:a + chunk]
        if not n_atoms:
            break
        dx, dy, dz = p[:, None, 0] - xyz[None, :, 0], p[:, None, 1] - xyz[None, :, 1], p[:, None, 2] - xyz[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        first = np.argmin(d2, axis=1)
        best = d2[np.arange(len(p)), first]
        d = np.sqrt(best)
        inside = d <= maxd
        owner[a:a + chunk] = np.where(inside, first, -1)
        tied[a:a + chunk] = inside & ((d2 == best[:, None]).sum(axis=1) >= 2)
        on_sphere[a:a + chunk] = d == maxd
    finite = np.isfinite(rho)          # (a NaN or infinite voxel is owned and counted, and enters no sum and neither filter)
    pos, neg = finite & (rho > cut), finite & (rho < -cut)
    out = {"owner": owner.reshape(int(header.uniqueNcrs[2]), int(header.uniqueNcrs[1]), int(header.uniqueNcrs[0])), "tied": tied, "on_sphere": on_sphere,
           "n": np.zeros(n_atoms, dtype=np.int64), "sum": np.zeros(n_atoms), "n_pos": np.zeros(n_atoms, dtype=np.int64), "sum_pos": np.zeros(n_atoms),
           "n_neg": np.zeros(n_atoms, dtype=np.int64), "sum_neg": np.zeros(n_atoms)}
    order = np.argsort(owner, kind="stable")
    bounds = np.searchsorted(owner[order], np.arange(-1, n_atoms + 1))

    def sums(mine):
        return (len(mine), math.fsum(rho[mine[finite[mine]]].tolist()), int(pos[mine].sum()), math.fsum(rho[mine[pos[mine]]].tolist()),
                int(neg[mine].sum()), math.fsum(rho[mine[neg[mine]]].tolist()))

    for k in range(n_atoms):
        mine = order[bounds[k + 1]:bounds[k + 2]]
        out["n"][k], out["sum"][k], out["n_pos"][k], out["sum_pos"][k], out["n_neg"][k], out["sum_neg"][k] = sums(mine)
    free = order[bounds[0]:bounds[1]]
    n, total, n_pos, total_pos, n_neg, total_neg = sums(free)
    out["unowned_n"] = np.array([n, n_pos, n_neg], dtype=np.int64)
    out["unowned_sum"] = np.array([total, total_pos, total_neg, math.fsum((rho[free[finite[free]]] ** 2).tolist())])
    return out
