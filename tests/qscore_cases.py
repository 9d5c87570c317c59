"""The inputs of the Q-score tests (shared by tests/test_qscore_host.py, which checks their conditioning, and
tests/test_gpu_qscore.py): seeded, so both see the same coordinates."""
import zlib

import numpy as np

from conftest import VOXEL_CASES

STEP, SIGMA, SHELLS, POINTS, LEVELS = 0.1, 0.6, 21, 8, 4      # DensityMatrix.qScores' defaults: R_max 2.0 A, reach 4.0 A
QS_STAGE = 128                                                # pdb_eda_amd/csrc/pdbeda_qscore.h
GOLDEN_MAPS = list(VOXEL_CASES)


def tables(shells=SHELLS, points=POINTS, levels=LEVELS, step=STEP):
    from pdb_eda_amd import ccp4
    return ccp4.qScoreTables(SIGMA, step, shells, points, levels)


def box_corners(header):
    return np.array([header.crs2xyzCoord([c, r, s]) for c in (0, header.ncrs[0] - 1) for r in (0, header.ncrs[1] - 1) for s in (0, header.ncrs[2] - 1)], dtype=np.float64)


def chain(name, header, n=300, bond=1.5, margin=2.0):
    """``n`` atoms at protein-like spacing: a seeded random walk of ``bond``-long steps, kept inside the xyz bounding box of the stored
    box grown by ``margin`` on every side (so some atoms sit outside the stored box, and on skewed cells many do)."""
    rng = np.random.default_rng(zlib.crc32(("qscore " + name).encode()))
    corners = box_corners(header)
    lo, hi = corners.min(axis=0) - margin, corners.max(axis=0) + margin
    at = rng.uniform(lo, hi)
    out = [at]
    while len(out) < n:
        step = rng.normal(size=3)
        nxt = at + bond * step / np.linalg.norm(step)
        if np.all(nxt >= lo) and np.all(nxt <= hi):
            out.append(nxt)
            at = nxt
    return np.array(out, dtype=np.float64)


def middle(header):
    """The coordinate of the stored box's middle voxel."""
    return np.array(header.crs2xyzCoord([int(header.ncrs[k]) // 2 for k in range(3)]), dtype=np.float64)


def shell_cluster(centre, count, radius, seed):
    """``count`` seeded atoms spread over the sphere of ``radius`` around ``centre`` (distinct coordinates)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(count, 3))
    return centre + radius * u / np.linalg.norm(u, axis=1)[:, None]


def crowded(header, extra, far=False):
    """An atom near the middle voxel (index 0), four atoms bonded to it at 1.5 A (indices 1 .. 4), and ``extra`` more spread over the
    sphere of 4 (1 + 5e-7) A around it: NEIGHBOURS of atom 0 (within the reach 2 R_max (1 + 1e-6) = 4 (1 + 1e-6) A, so the kernel has
    to stage or walk them) that can win none of its sample points (they are more than 2 R_max away: R_max from every point).  With
    ``far`` the same atoms sit on the sphere of 4 (1 + 2e-6) A, outside the reach: atom 0 must come out the same to the bit."""
    centre = middle(header) + np.array([0.05, -0.07, 0.11])
    bonded = centre + 1.5 * np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])
    return np.concatenate([centre[None, :], bonded, shell_cluster(centre, extra, 4.0 * (1.0 + (2e-6 if far else 5e-7)), 1234 + extra)])
