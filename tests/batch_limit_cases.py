"""The maps and atoms of tests/test_gpu_batch_limits.py, seeded, so that the test and the child process of its
PDBEDA_COPY_KERNELS=0 case see the same bytes: two small synthetic maps and P distinct atom positions that are tiled to
the batch size."""
import numpy as np

import profiles_cases

P = 3001          # distinct positions: a prime, so atoms v and v + 65536 differ and groups repeat with a period coprime to 1024
WORLDS = ["orth", "skew"]


def spec_and_grid(name):
    """orth: 48 x 40 x 36 at 0.5 A, the whole cell stored (every wrapped voxel exists: `valid` is always true).
    skew: a triclinic cell with permuted axes, crsStart != 0 and an interval 7 voxels longer than ncrs along one axis (the
    arguments of tools/soak_spheres.py's fourth kind of cell, on skewed angles): part of the cell is not stored, so `valid` has both answers."""
    from pdb_eda_amd import synthetic
    ncrs = (48, 40, 36)
    if name == "orth":
        spec = synthetic.MapSpec(ncrs=ncrs, spacing=0.5)
    else:
        order, extra = (3, 1, 2), (0, 7, 0)
        interval = [0, 0, 0]
        for crs_axis, xyz_axis in enumerate(order):
            interval[xyz_axis - 1] = ncrs[crs_axis] + extra[crs_axis]
        spec = synthetic.MapSpec(ncrs=ncrs, spacing=0.5, angles=(82.0, 97.0, 110.0), axis_order=order, interval=interval, crs_start=(4, -2, 0))
    return spec, synthetic.smooth_noise((ncrs[2], ncrs[1], ncrs[0]), 4100 + WORLDS.index(name))


def base_atoms(name, header):
    """P distinct positions: random ones from 4 voxels outside the stored box on every side and some exactly on voxel centres
    (profiles_cases.case_atoms); every fourth random position is then moved to within 0.5 A per axis of the one before it, so
    that consecutive positions give spheres that overlap as well as spheres that lie apart."""
    xyz = profiles_cases.case_atoms("batch_limits_" + name, header, n_random=P - 200, n_centres=260)
    rng = np.random.default_rng(977 + WORLDS.index(name))
    near = np.arange(1, P - 200, 4)
    xyz[near] = xyz[near - 1] + rng.uniform(-0.5, 0.5, size=(len(near), 3))
    _, first = np.unique(xyz, axis=0, return_index=True)
    xyz = xyz[np.sort(first)][:P]
    assert len(xyz) == P
    return np.ascontiguousarray(xyz)


def tiled(n):
    """Atom i of a batch of n sits on position i % P."""
    return np.arange(n) % P
