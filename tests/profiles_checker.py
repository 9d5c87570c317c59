"""The radial-profile contract of include/pdbeda.h (pdbeda_radial_profiles) restated in plain numpy: the yardstick of
tests/test_gpu_profiles.py.  Nothing here comes from the product's native library: the box is made with the header's
xyz2crsCoord, the voxel coordinates with its crs2xyzCoord (or a callable the caller hands in), the wrap rule is written out,
the shells are numpy fp64 ``/`` and ``floor``, and the sums are math.fsum (exact, then rounded once)."""
import math

import numpy as np


def sphere_box(header, xyz, radius):
    """[C - R - 1, C + R] per crs axis (inclusive): C = xyz2crsCoord(atom), R = xyz2crsCoord(origin + radius), radius in float32."""
    rad = float(np.float32(radius))
    C = header.xyz2crsCoord([float(v) for v in xyz])
    R = header.xyz2crsCoord([header.origin[i] + rad for i in range(3)])
    return [C[k] - R[k] - 1 for k in range(3)], [C[k] + R[k] for k in range(3)]


def box_voxels(lo, hi):
    """The raw crs triples of a box, c fastest (n x 3 int64); empty along any axis: no voxel."""
    if any(hi[k] < lo[k] for k in range(3)):
        return np.zeros((0, 3), dtype=np.int64)
    s, r, c = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
    return np.stack([c.reshape(-1), r.reshape(-1), s.reshape(-1)], axis=1).astype(np.int64)


def point_density(header, grid, crs):
    """getPointDensityFromCrs / testValidCrs on an (n x 3) array: per axis, a coordinate outside [0, ncrs) is wrapped by the
    axis's interval (floor modulo); one that then lies in [ncrs, interval) is not stored: density 0, not valid."""
    ok = np.ones(len(crs), dtype=bool)
    idx = []
    for k in range(3):
        v = crs[:, k].copy()
        n, interval = int(header.ncrs[k]), int(header.crsInterval[k])
        outside = (v < 0) | (v >= n)
        v[outside] = np.mod(v[outside], interval)          # (numpy's mod is Python's: the sign of the divisor)
        ok &= ~(((n <= v) & (v < interval)) | (v < 0))
        idx.append(v)
    rho = np.zeros(len(crs), dtype=np.float64)
    rho[ok] = grid[idx[2][ok], idx[1][ok], idx[0][ok]].astype(np.float64)
    return rho, ok


def radial_profiles(header, grid, xyz, radius, n_shells, cutoff, crs2xyz=None):
    """Per atom and shell: n, sum, n_sig, sum_sig ((n_atoms, n_shells)); per atom: valid, and boundary_ties = the voxels inside
    the sphere (d > 0) whose d / w is a whole number -- they sit exactly on a shell boundary.
    crs2xyz: (n x 3 integer array) -> (n x 3 float64 array); default: header.crs2xyzCoord, voxel by voxel."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    grid = np.asarray(grid, dtype=np.float32).reshape(header.ncrs[2], header.ncrs[1], header.ncrs[0])
    rad, cut = float(np.float32(radius)), float(np.float32(cutoff))
    w = np.float64(rad) / np.float64(n_shells)
    boxes = [box_voxels(*sphere_box(header, p, radius)) for p in xyz]
    every = np.concatenate(boxes) if boxes else np.zeros((0, 3), dtype=np.int64)
    if crs2xyz is None:
        where = np.array([header.crs2xyzCoord([int(v) for v in crs]) for crs in every], dtype=np.float64).reshape(-1, 3)
    else:
        where = np.asarray(crs2xyz(every.astype(np.int32)), dtype=np.float64).reshape(-1, 3)
    shape = (len(xyz), n_shells)
    out = {"n": np.zeros(shape, dtype=np.int64), "sum": np.zeros(shape), "n_sig": np.zeros(shape, dtype=np.int64), "sum_sig": np.zeros(shape),
           "valid": np.ones(len(xyz), dtype=bool), "boundary_ties": np.zeros(len(xyz), dtype=np.int64)}
    at = 0
    for a, crs in enumerate(boxes):
        p = where[at:at + len(crs)]
        at += len(crs)
        dx, dy, dz = p[:, 0] - xyz[a, 0], p[:, 1] - xyz[a, 1], p[:, 2] - xyz[a, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        inside = d <= rad
        crs, d = crs[inside], d[inside]
        rho, ok = point_density(header, grid, crs)
        q = d / w
        shell = np.minimum(np.floor(q).astype(np.int64), n_shells - 1)
        sig = rho > cut if cut > 0 else (rho < cut if cut < 0 else np.ones(len(rho), dtype=bool))
        out["valid"][a] = bool(ok.all())
        out["boundary_ties"][a] = int(np.count_nonzero((q == np.floor(q)) & (d > 0)))
        for k in range(n_shells):
            mine = shell == k
            out["n"][a, k] = int(np.count_nonzero(mine))
            out["sum"][a, k] = math.fsum(rho[mine].tolist())
            out["n_sig"][a, k] = int(np.count_nonzero(mine & sig))
            out["sum_sig"][a, k] = math.fsum(rho[mine & sig].tolist())
    return out
