"""The atoms the radial-profile tests place on the voxel goldens (shared by tests/test_profiles_host.py and
tests/test_gpu_profiles.py): seeded, so both see the same coordinates."""
import zlib

import numpy as np


def case_atoms(name, header, n_random=24, n_centres=8):
    """(n_random + n_centres) x 3 float64: random positions from 4 voxels outside the stored box on every side, and positions
    exactly on voxel centres (header.crs2xyzCoord of integer crs, some of them outside the stored box too; the first is the middle
    voxel of the stored box, whose sphere of 3.5 A lies inside every golden's stored box)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ncrs = np.asarray(header.ncrs, dtype=np.float64)
    frac = rng.uniform(-4.0, ncrs + 4.0, size=(n_random, 3))
    random_xyz = header.crs2xyz_array(frac)
    crs = np.stack([rng.integers(-3, int(header.ncrs[k]) + 3, size=n_centres) for k in range(3)], axis=1)
    if n_centres:
        crs[0] = [int(header.ncrs[k]) // 2 for k in range(3)]
    centre_xyz = np.array([header.crs2xyzCoord([int(v) for v in c]) for c in crs], dtype=np.float64).reshape(-1, 3)
    return np.concatenate([random_xyz, centre_xyz])
