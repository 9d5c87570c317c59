"""The atoms the partition tests place on the voxel goldens (shared by tests/test_partition_host.py and
tests/test_gpu_partition.py): seeded, so both see the same coordinates."""
import numpy as np

import profiles_cases


def random(name, header):
    """32 atoms: profiles_cases.case_atoms -- random positions in and around the stored box, and positions exactly on voxel centres."""
    return profiles_cases.case_atoms(name, header)


def lattice(header):
    """Atoms exactly on voxel centres at every 4th voxel from 2 of the non-repeating box (orth_rep: 294 atoms): with a voxel spacing
    that is exact in binary, the voxels half way between two of them are equidistant to the bit, and whole shells of voxels lie
    exactly on a sphere."""
    axes = [range(2, int(header.uniqueNcrs[k]), 4) for k in range(3)]
    return np.array([header.crs2xyzCoord([c, r, s]) for s in axes[2] for r in axes[1] for c in axes[0]], dtype=np.float64).reshape(-1, 3)
