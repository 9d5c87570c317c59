"""The per-atom region-sum contract of include/pdbeda.h (pdbeda_region_sums) restated in plain numpy: the yardstick of
tests/test_gpu_batch_limits.py, pinned against the oracle by tests/test_spheres_host.py.  The box, the box's voxels and the
wrapped fetch are tests/profiles_checker.py's (sphere_box, box_voxels, point_density); the voxel coordinates are the header's
crs2xyzCoord or a callable the caller hands in; nothing else comes from the product's native library.  Vectorised over atoms:
the atoms of one radius have boxes of one shape, so they are one (n_atoms, n_box, 3) crs array, one distance test and one
wrapped gather; the sums are numpy's pairwise fp64 sums along the box axis."""
import numpy as np

import profiles_checker


def atom_spheres(header, grid, xyz, radii, crs2xyz=None):
    """Per atom, the voxels of its sphere in box order (c fastest), every atom's after the one before: a dict of ``crs``
    (n x 3 int64, raw), ``rho`` (n, float64: 0 where nothing is stored), ``ok`` (n, bool: stored) and ``offsets``
    (n_atoms + 1): atom a's voxels are rows offsets[a]:offsets[a + 1].
    radii: one per atom, or one for all;  crs2xyz: (n x 3 integer array) -> (n x 3 float64 array); default: header.crs2xyzCoord."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(xyz),))
    grid = np.asarray(grid, dtype=np.float32).reshape(header.ncrs[2], header.ncrs[1], header.ncrs[0])
    parts = {"atom": [], "crs": [], "rho": [], "ok": []}
    for radius in np.unique(radii):
        mine = np.nonzero(radii == radius)[0]
        boxes = [profiles_checker.sphere_box(header, xyz[a], radius) for a in mine]
        lo = np.array([b[0] for b in boxes], dtype=np.int64)
        shape = [boxes[0][1][k] - boxes[0][0][k] for k in range(3)]          # (hi - lo = 2 R + 1 per axis: the radius alone decides it)
        template = profiles_checker.box_voxels([0, 0, 0], shape)
        crs = lo[:, None, :] + template[None, :, :]
        flat = crs.reshape(-1, 3)
        if crs2xyz is None:
            where = np.array([header.crs2xyzCoord([int(v) for v in c]) for c in flat], dtype=np.float64).reshape(-1, 3)
        else:
            where = np.asarray(crs2xyz(flat.astype(np.int32)), dtype=np.float64).reshape(-1, 3)
        where = where.reshape(len(mine), len(template), 3)
        dx, dy, dz = (where[:, :, k] - xyz[mine, k][:, None] for k in range(3))
        inside = (np.sqrt((dx * dx + dy * dy) + dz * dz) <= float(radius)).reshape(-1)
        rho, ok = profiles_checker.point_density(header, grid, flat[inside])
        parts["atom"].append(np.repeat(mine, len(template))[inside])
        parts["crs"].append(flat[inside])
        parts["rho"].append(rho)
        parts["ok"].append(ok)
    cat = lambda k, dtype, tail: np.concatenate(parts[k]) if parts[k] else np.zeros((0,) + tail, dtype=dtype)
    atom = cat("atom", np.int64, ())
    order = np.argsort(atom, kind="stable")          # atom order; within an atom the box order stays
    counts = np.bincount(atom, minlength=len(xyz)).astype(np.int64)
    return {"crs": cat("crs", np.int64, (3,))[order], "rho": cat("rho", np.float64, ())[order], "ok": cat("ok", bool, ())[order],
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}


def _sums(rho, ok, offsets, cutoff):
    """cnt, pos, neg, valid per segment offsets[g]:offsets[g + 1] of rho / ok: a padded (n_segments, longest) array, summed along
    the segment (numpy's pairwise fp64 sum of a contiguous row); the comparisons against float32(cutoff), strict."""
    cut = float(np.float32(cutoff))
    cnt = np.diff(offsets)
    width = int(cnt.max()) if len(cnt) else 0
    cols = np.arange(width)[None, :]
    filled = cols < cnt[:, None]
    at = np.minimum(offsets[:-1, None] + cols, max(len(rho) - 1, 0))
    padded = np.where(filled, rho[at], 0.0) if len(rho) else np.zeros(filled.shape)
    stored = np.where(filled, ok[at], True) if len(rho) else np.ones(filled.shape, dtype=bool)
    return {"cnt": cnt.astype(np.int64), "pos": np.where(padded > cut, padded, 0.0).sum(axis=1), "neg": np.where(padded < -cut, padded, 0.0).sum(axis=1),
            "n_pos": np.count_nonzero(filled & (padded > cut), axis=1), "n_neg": np.count_nonzero(filled & (padded < -cut), axis=1),
            "valid": stored.all(axis=1)}


def region_sums(header, grid, xyz, radii, cutoff, group_offsets=None, crs2xyz=None, spheres=None):
    """pdbeda_region_sums: per group ``cnt`` (voxels of the union of its atoms' spheres, no density filter), ``pos`` (sum of
    rho > cut), ``neg`` (sum of rho < -cut), ``n_pos`` / ``n_neg`` (the voxels in those sums), ``valid`` (every voxel of every atom's sphere is stored).
    group_offsets None: a group per atom.  spheres: what atom_spheres returned for these atoms (computed once, used for several cutoffs)."""
    sp = atom_spheres(header, grid, xyz, radii, crs2xyz) if spheres is None else spheres
    if group_offsets is None:
        return _sums(sp["rho"], sp["ok"], sp["offsets"], cutoff)
    goff = np.asarray(group_offsets, dtype=np.int64)
    rho, ok, counts, valid = [], [], [], []
    for g in range(len(goff) - 1):          # the set union on raw crs (a voxel two atoms of the group share counts once)
        a, b = int(sp["offsets"][goff[g]]), int(sp["offsets"][goff[g + 1]])
        _, first = np.unique(sp["crs"][a:b], axis=0, return_index=True)
        rho.append(sp["rho"][a:b][first])
        ok.append(sp["ok"][a:b][first])
        counts.append(len(first))
        valid.append(bool(sp["ok"][a:b].all()))          # the conjunction over the atoms
    out = _sums(np.concatenate(rho) if rho else np.zeros(0), np.concatenate(ok) if ok else np.zeros(0, dtype=bool),
                np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), cutoff)
    assert np.array_equal(out["valid"], np.array(valid, dtype=bool))          # (a voxel's `ok` does not depend on the atom that reached it)
    return out


def group_voxels(spheres, group_offsets=None):
    """Per group, the set of raw crs triples of the union of its atoms' spheres (membership, for comparison with the oracle's lists)."""
    n_atoms = len(spheres["offsets"]) - 1
    goff = np.arange(n_atoms + 1) if group_offsets is None else np.asarray(group_offsets, dtype=np.int64)
    return [{tuple(int(x) for x in v) for v in spheres["crs"][int(spheres["offsets"][goff[g]]):int(spheres["offsets"][goff[g + 1]])]}
            for g in range(len(goff) - 1)]
