"""The maps, fragments, rotations and centres of the pose-score tests (shared by tests/test_pose_host.py, tests/test_pose_plan_host.py and
tests/test_gpu_pose.py): seeded, so all see the same numbers.  A case is a dict: ``tag``, ``map`` (a name of MAPS), ``frag`` (n, 3), ``w``
(n,), ``rot`` (n_rot, 3, 3), ``centres`` (n, 3), ``top_k``, ``floor``, ``max_low``, ``allow_outside``, ``ranked`` (the case checks ranking:
tests/test_pose_host.py holds it to "a centre with kept poses and a centre with a rejected pose").

Maps (24^3 .. 30^3 unless said otherwise; uniform in [-1, 1]): ``orth`` a whole orthogonal cell (it repeats); ``cut`` a cut-out with crsStart
!= 0 (beyond its faces nothing is stored); ``rep`` stored box larger than the cell along c; ``perm`` permuted axes; ``hex`` the skewed cell,
a cut-out; ``nan`` orth with a NaN and an inf voxel; ``half`` orth, +1 +- 0.1 in one half and -1 +- 0.1 in the other; ``fine`` 8^3 voxels of
0.25 A that repeat (a box wraps it more than three times).

The default low-atom rule, floor 0 and max_low n_frag // 2, rejects about half the poses of a random map and keeps the rest."""
import io

import numpy as np

from pdb_eda_amd import ccp4, synthetic

MAPS = {
    "orth": dict(ncrs=(24, 26, 28), spacing=0.5),
    "cut": dict(ncrs=(24, 20, 22), crs_start=(-3, 5, 2), interval=(40, 36, 30), spacing=0.4),
    "rep": dict(ncrs=(30, 24, 24), interval=(24, 24, 24), spacing=0.5),
    "perm": dict(ncrs=(26, 30, 22), crs_start=(4, 0, -6), axis_order=(2, 3, 1), spacing=0.42),
    "hex": dict(ncrs=(28, 26, 24), angles=(90.0, 90.0, 120.0), axis_order=(2, 1, 3), crs_start=(-5, 3, 7), interval=(32, 36, 30), cell=(14.4, 14.4, 12.0)),
    "nan": dict(ncrs=(24, 26, 28), spacing=0.5),
    "half": dict(ncrs=(24, 24, 24), spacing=0.5),
    "cube": dict(ncrs=(24, 24, 24), spacing=0.5),
    "fine": dict(ncrs=(8, 8, 8), spacing=0.25),
}
NAN_AT, INF_AT = (5, 6, 7), (15, 16, 17)      # (s, r, c) of the two voxels of ``nan``
_headers, _grids = {}, {}


def spec_of(name):
    return synthetic.MapSpec(**MAPS[name])


def grid_of(name):
    if name not in _grids:
        nc, nr, ns = MAPS[name]["ncrs"]
        rng = np.random.default_rng(sum(ord(ch) for ch in name) + 101)
        g = rng.uniform(-1.0, 1.0, size=(ns, nr, nc)).astype(np.float32)
        if name == "nan":
            g[NAN_AT], g[INF_AT] = np.float32(np.nan), np.float32(np.inf)
        if name == "half":
            g = (np.where(np.arange(nc)[None, None, :] < nc // 2, 1.0, -1.0) + 0.1 * g).astype(np.float32)
        _grids[name] = g
    return _grids[name]


def map_bytes(name):
    return synthetic.ccp4_bytes(spec_of(name), grid_of(name))


def header_of(name):
    if name not in _headers:
        _headers[name] = ccp4.read_grid(io.BytesIO(map_bytes(name)))[0]
    return _headers[name]


def voxel(name, c, r, s, shift=(0.0, 0.0, 0.0)):
    return np.array(header_of(name).crs2xyzCoord([c, r, s]), dtype=np.float64) + np.asarray(shift, dtype=np.float64)


def fragment(n, radius=2.0, seed=3):
    """``n`` atoms in the ball of ``radius``, relative to their centroid; weights in [1, 8]."""
    rng = np.random.default_rng(seed + n)
    u = rng.normal(size=(n, 3))
    x = u / np.linalg.norm(u, axis=1)[:, None] * (radius * np.cbrt(rng.uniform(0.05, 1.0, size=n)))[:, None]
    return x - x.mean(axis=0), rng.uniform(1.0, 8.0, size=n)


def rod(half_length, n_inner=5, seed=9):
    """Two atoms at +-half_length along x exactly (the radius IS half_length) and ``n_inner`` atoms within 1 A of the pivot."""
    inner = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(n_inner, 3))
    return np.concatenate([[[half_length, 0.0, 0.0], [-half_length, 0.0, 0.0]], inner]), np.ones(n_inner + 2)


def interior(name, n, seed=17):
    """``n`` seeded centres in the middle third of the stored box."""
    h = header_of(name)
    rng = np.random.default_rng(seed)
    nc, nr, ns = (int(v) for v in h.ncrs)
    return np.array([voxel(name, int(rng.integers(nc // 3, 2 * nc // 3)), int(rng.integers(nr // 3, 2 * nr // 3)), int(rng.integers(ns // 3, 2 * ns // 3)),
                           rng.uniform(-0.2, 0.2, size=3)) for _ in range(n)])


def case(tag, name, frag_w, n_rot, centres, top_k=3, floor=0.0, max_low="half", allow_outside=False, ranked=True, rot=None):
    frag, w = frag_w
    return {"tag": tag, "map": name, "frag": np.asarray(frag, dtype=np.float64), "w": np.asarray(w, dtype=np.float64),
            "rot": ccp4.rotationLattice(n_rot) if rot is None else np.asarray(rot, dtype=np.float64), "centres": np.asarray(centres, dtype=np.float64).reshape(-1, 3),
            "top_k": top_k, "floor": floor, "max_low": (len(w) // 2 if max_low == "half" else max_low), "allow_outside": allow_outside, "ranked": ranked}


def cases():
    out = []
    # the geometries; fragment sizes 1, 2, 7, 64, 65 and the cap; rotation counts 1, 63, 64, 65, 257
    on_voxel, far = voxel("orth", 7, 9, 11), voxel("orth", 7 + 5 * 24, 9 - 3 * 26, 11 + 2 * 28, (0.11, -0.07, 0.13))      # (a voxel centre; five cells away: it wraps)
    out.append(case("orth-7-257", "orth", fragment(7), 257, np.concatenate([[on_voxel, far], interior("orth", 4)]), top_k=5))
    last = voxel("cut", 23, 19, 21)                                                                                   # the last stored voxel: atoms fall outside
    out.append(case("cut-7-65", "cut", fragment(7), 65, np.concatenate([interior("cut", 2), [last]]), top_k=3))
    out.append(case("cut-7-65-outside", "cut", fragment(7), 65, np.concatenate([interior("cut", 2), [last]]), top_k=3, allow_outside=True))
    out.append(case("rep-2-64", "rep", fragment(2), 64, np.concatenate([interior("rep", 3), [voxel("rep", 29, 23, 23, (0.1, 0.1, 0.1))]]), top_k=1))
    out.append(case("perm-64-63", "perm", fragment(64), 63, interior("perm", 3), top_k=64))                       # top_k at its cap, above the 63 poses
    out.append(case("hex-65-65", "hex", fragment(65), 65, interior("hex", 3), top_k=4))
    out.append(case("hex-7-257", "hex", fragment(7, 1.5), 257, np.concatenate([interior("hex", 3), [voxel("hex", 27, 25, 23)]]), top_k=5))
    out.append(case("orth-cap-63", "orth", fragment(256, 3.0), 63, interior("orth", 2), top_k=2))
    out.append(case("orth-1-1", "orth", fragment(1), 1, interior("orth", 8, seed=5), top_k=3, max_low=0))         # more rows than poses: -1 / +0.0 fill
    # non-finite voxels: a centre on the NaN voxel (every pose NaN: rejected), one on the inf voxel, others far from both
    s, r, c = NAN_AT
    s2, r2, c2 = INF_AT
    out.append(case("nan-7-64", "nan", fragment(7, 1.0), 64, np.concatenate([[voxel("nan", c, r, s), voxel("nan", c2, r2, s2)], [voxel("nan", 12, 3, 22, (0.1, 0.2, 0.05))]]),
                    top_k=3, floor=-np.inf, max_low=None))
    # ties: every atom on the pivot (all rotations tie at every centre); the identity listed twice with a centrosymmetric fragment
    out.append(case("pivot-3-64", "orth", (np.zeros((3, 3)), [1.0, 2.0, 3.0]), 64, np.concatenate([interior("orth", 3), [on_voxel]]), top_k=5,
                    floor=float(grid_of("orth")[11, 9, 7]) + 0.01))                                                  # (the voxel-centre centre reads below the floor: rejected)
    half, hw = fragment(4, 1.5)
    twice = np.concatenate([np.eye(3)[None], np.eye(3)[None], ccp4.rotationLattice(5)])
    out.append(case("centro-8-7", "orth", (np.concatenate([half, -half]), np.concatenate([hw, hw])), 7, interior("orth", 4, seed=23), top_k=7, rot=twice,
                    floor=-np.inf, max_low=None, ranked=False))
    # weights with zeros and negatives
    fx, _ = fragment(7)
    out.append(case("weights-7-65", "orth", (fx, [0.0, -1.5, 2.0, -0.0, 3.0, -4.0, 1.0]), 65, interior("orth", 3), top_k=4))
    # the low-atom rule: max_low 0 and floor 0 reject every pose in the negative half and none in the positive half
    out.append(case("half-low", "half", fragment(7, 1.5), 64, [voxel("half", 6, 12, 12, (0.1, 0.1, 0.1)), voxel("half", 18, 12, 12, (0.1, 0.1, 0.1))], top_k=3, max_low=0))
    # the staging edge on 24^3 voxels of 0.5 A, centres on voxel centres: a radius of 13 voxels gives a box of 31^3 (122 892 bytes: staged), one
    # of 14 voxels 33^3 (148 236 bytes: global); either box is wider than the map and wraps it
    at = [voxel("cube", 12, 12, 12), voxel("cube", 3, 20, 7)]
    out.append(case("stage-fits", "cube", rod(6.5), 64, at, top_k=3))
    out.append(case("stage-exceeds", "cube", rod(7.0), 64, at, top_k=3))
    out.append(case("fine-wraps", "fine", rod(3.0), 65, [voxel("fine", 3, 4, 5, (0.05, 0.02, 0.07)), voxel("fine", 0, 0, 0)], top_k=3))
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = cases()
    return _cases


def find(tag):
    return [c for c in all_cases() if c["tag"] == tag][0]
