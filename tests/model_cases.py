"""The maps and atoms of the model-density tests (shared by tests/test_model_host.py and tests/test_gpu_model.py): seeded, so both see the
same numbers.  A case is (MapSpec, xyz, amp [n][terms], expo [n][terms], radii float32).

How the numbers are chosen.  The GPU test wants every voxel within ONE float32 spacing of the exact value.  Before its last rounding a
voxel of k terms is off by at most k * 2^-41 (S = 40).  If every term is at least t_min and all have one sign, the voxel is at least
k t_min and its float32 spacing at least 2^-24 k t_min: k 2^-41 is below a thousandth of half that spacing once t_min >= 2^-14.  Hence
amplitudes in [0.5, 2] and expo * radius^2 <= 6 (a last term >= 0.5 e^-6 = 1.2e-3), and negative amplitudes only where they cancel a
coincident term exactly (the integers then add up to exactly 0) or take a fixed quarter of it (the sum keeps its sign and three
quarters of its size).  tests/test_model_host.py checks t_min and that no pair lies within 1e-9 of its sphere."""
import io

import numpy as np

from pdb_eda_amd import ccp4, synthetic

STAGE = 256                 # MD_STAGE of pdb_eda_amd/csrc/pdbeda_model.h
TILE = (16, 4, 4)           # PT_C, PT_R, PT_S

SPECS = {
    "box": dict(ncrs=(21, 9, 7), spacing=0.5),                                                  # no multiple of the tile on any axis
    "skew": dict(ncrs=(21, 9, 7), angles=(90.0, 90.0, 120.0), axis_order=(2, 1, 3), crs_start=(3, -2, 5), interval=(16, 32, 12), cell=(8.0, 16.0, 6.0)),
    "rep": dict(ncrs=(21, 9, 7), interval=(16, 9, 7), spacing=0.5),                            # stored box larger than the unique box along c
    "tile": dict(ncrs=TILE, spacing=0.5),                                                       # one exact tile
    "past": dict(ncrs=(17, 5, 5), spacing=0.5),                                                 # one voxel past a tile on every axis
    "wide": dict(ncrs=(48, 12, 12), spacing=0.5),                                               # 27 tiles: neighbours stage different atoms
}
_headers = {}


def spec_of(name):
    return synthetic.MapSpec(**SPECS[name])


def header_of(name):
    if name not in _headers:
        spec = spec_of(name)
        nc, nr, ns = spec.ncrs
        _headers[name] = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((ns, nr, nc), dtype=np.float32))))[0]
    return _headers[name]


def box_of(name):
    """(lo, hi) of the stored voxels' coordinates."""
    h = header_of(name)
    nc, nr, ns = (int(v) for v in h.ncrs)
    corners = np.array([h.crs2xyzCoord([c, r, s]) for c in (0, nc - 1) for r in (0, nr - 1) for s in (0, ns - 1)], dtype=np.float64)
    return corners.min(axis=0), corners.max(axis=0)


def _terms(rng, n, n_terms, radii):
    amp = rng.uniform(0.5, 2.0, size=(n, n_terms))
    expo = rng.uniform(1.0, 6.0, size=(n, n_terms)) / (radii.astype(np.float64) ** 2)[:, None]
    return amp, expo


def scattered(name, n=40, n_terms=1, seed=11):
    """Atoms in and around the stored box (up to 2 A outside it: their spheres reach in), radii 0.6 .. 2.4 (4x), two far away that reach
    nothing, and three that share one coordinate."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(name)
    xyz = rng.uniform(lo - 2.0, hi + 2.0, size=(n, 3))
    xyz[-3:] = xyz[-4]                                              # coincident atoms
    xyz[0] = hi + 100.0                                             # far away
    xyz[1] = lo - 250.0
    xyz[2] = [lo[0] - 1.0, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]          # outside, reaching in with the largest radius
    radii = rng.uniform(0.6, 2.4, size=n).astype(np.float32)
    radii[2], radii[3] = np.float32(2.4), np.float32(0.6)
    amp, expo = _terms(rng, n, n_terms, radii)
    if n_terms == 6:                                                # a negative term that takes a quarter of term 0: same exponent, the sum stays positive
        amp[:, 5], expo[:, 5] = -0.25 * amp[:, 0], expo[:, 0]
    return xyz, amp, expo, radii


def clustered(name, n, seed=5):
    """n atoms inside a 1 A cube in the middle of the first tile: that tile stages all of them."""
    rng = np.random.default_rng(seed + n)
    h = header_of(name)
    mid = np.array(h.crs2xyzCoord([7, 2, 2]), dtype=np.float64)
    xyz = mid + rng.uniform(-0.5, 0.5, size=(n, 3))
    radii = rng.uniform(0.8, 1.5, size=n).astype(np.float32)
    amp, expo = _terms(rng, n, 1, radii)
    return xyz, amp, expo, radii


def spread(name="wide", n=300, seed=3):
    """Atoms all over a box of 27 tiles with radii of 0.6 .. 0.9: the cells are small and no tile stages them all."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(name)
    xyz = rng.uniform(lo - 0.5, hi + 0.5, size=(n, 3))
    radii = rng.uniform(0.6, 0.9, size=n).astype(np.float32)
    amp, expo = _terms(rng, n, 1, radii)
    return xyz, amp, expo, radii


def cancelling(name, seed=17):
    """Pairs of coincident atoms: +a / -a with one exponent and one radius (exactly nothing), and +a / -a/4 with the smaller radius on the
    negative one (a inside the shell between the radii, 3a/4 inside the smaller)."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(name)
    base = rng.uniform(lo + 0.5, hi - 0.5, size=(6, 3))
    radii = rng.uniform(0.8, 1.6, size=6).astype(np.float32)
    amp, expo = _terms(rng, 6, 1, radii)
    xyz = np.concatenate([base, base])
    amp2 = np.concatenate([amp, -amp])
    amp2[9:] = -0.25 * amp[3:]
    radii2 = np.concatenate([radii, radii])
    radii2[9:] = (radii[3:] * np.float32(0.5)).astype(np.float32)
    return xyz, amp2, np.concatenate([expo, expo]), radii2


def on_sphere(name="box"):
    """One atom on a voxel centre with a radius of exactly three grid steps (1.5, a float32): the voxels three steps along an axis, and those at (2, 2, 1) steps, lie
    ON the sphere and belong to it.  expo = 0: the value is the amplitude everywhere inside."""
    h = header_of(name)
    xyz = np.array([h.crs2xyzCoord([10, 4, 3])], dtype=np.float64)
    return xyz, np.array([[0.75]]), np.array([[0.0]]), np.array([1.5], dtype=np.float32)


def conditioned_cases():
    """(tag, header name, atoms) of every GPU case that must not hinge on an ulp: all but the crafted on-sphere one."""
    out = [("scattered-%s-%d" % (name, nt), name, scattered(name, n_terms=nt)) for name in ("box", "skew", "rep", "tile", "past") for nt in (1, 6)]
    out += [("clustered-%d" % n, "box", clustered("box", n)) for n in (STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 3)]
    out += [("spread", "wide", spread()), ("cancelling", "box", cancelling("box"))]
    return out
