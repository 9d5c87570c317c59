"""The maps and atoms of the atom-moment tests (shared by tests/test_gradient_host.py and tests/test_gpu_gradient.py): seeded, on the
geometries of tests/model_cases.py.  A case is (tag, header name, weight kind, unique box?, xyz, expo [n][terms], radii float32).

What the atom lists cover: atoms in the interior; atoms whose sphere the domain clips on each of its six faces; atoms wholly outside; two
coincident atoms; one, three and six terms; expo = 0; radii from under one voxel (0.2 A on a 0.5 A grid) to 3 A; and boxes of the three
kinds the kernel's 16 x 4 trips see: at most 64 voxels, one trip plus one (5 rows: a second trip of one row; 17 columns: a second trip of
one column) and many trips.  No coordinate sits on a voxel centre and no radius is a multiple of the grid step:
tests/test_gradient_host.py checks that no pair lies within 1e-9 of its sphere.

Weight maps: ``zero``, ``one``, ``random`` (uniform in [-1, 1]) and ``spike`` (random with one voxel of 3e6, which moves S by 22)."""
import numpy as np

from model_cases import SPECS, spec_of, header_of, box_of      # noqa: F401  (the geometries are model_cases')

GEOMETRIES = ("box", "skew", "rep", "tile", "past", "wide")
SPIKE = 3.0e6


def weight(name, kind, seed=23):
    h = header_of(name)
    shape = (int(h.ncrs[2]), int(h.ncrs[1]), int(h.ncrs[0]))
    if kind == "zero":
        return np.zeros(shape, dtype=np.float32)
    if kind == "one":
        return np.ones(shape, dtype=np.float32)
    w = np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)
    if kind == "spike":
        w[shape[0] // 2, shape[1] // 2, shape[2] // 3] = np.float32(SPIKE)
    return w


def _expo(rng, n, n_terms, radii):
    expo = rng.uniform(0.5, 6.0, size=(n, n_terms)) / (radii.astype(np.float64) ** 2)[:, None]
    expo[0, 0] = 0.0                                                # the plain moments of the weight inside the sphere
    return expo


def atoms(name, n_terms=1, seed=41):
    """18 atoms: 6 inside, 6 reaching in over one face each, 2 wholly outside, 2 coincident, 1 under a voxel, 1 of 3 A."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(name)
    mid, span = 0.5 * (lo + hi), hi - lo
    inside = mid + rng.uniform(-0.25, 0.25, size=(6, 3)) * span
    faces = np.repeat(mid[None, :], 6, axis=0) + rng.uniform(-0.1, 0.1, size=(6, 3)) * span
    for k in range(3):
        faces[2 * k, k] = lo[k] - 0.37
        faces[2 * k + 1, k] = hi[k] + 0.41
    outside = np.array([hi + 100.0, lo - 250.0])
    twin = mid + rng.uniform(-0.2, 0.2, size=3) * span
    small = mid + np.array([0.013, 0.021, -0.017])
    large = mid + np.array([-0.31, 0.17, 0.23])
    xyz = np.concatenate([inside, faces, outside, [twin, twin], [small], [large]])
    radii = np.concatenate([rng.uniform(0.6, 2.0, size=6), rng.uniform(0.9, 1.9, size=6), [1.3, 0.7], [1.23, 1.23], [0.2], [3.0]]).astype(np.float32)
    return xyz, _expo(rng, len(xyz), n_terms, radii), radii


def trips(name="wide"):
    """Five atoms near voxel centres of ``wide`` whose covering boxes are 3 x 3 x 3 (27 voxels: less than a trip), 5 x 5 x 5 (two trips of rows,
    the second of one row), 17 x 12 x 12 (two trips of columns, the second of one column; a radius of 4.1 A, clipped along r and s), 13 x 12 x 12 and
    11 x 11 x 11 (many trips)."""
    h = header_of(name)
    centre = lambda c, r, s, d: np.array(h.crs2xyzCoord([c, r, s]), dtype=np.float64) + d
    xyz = np.array([centre(8, 5, 5, [0.013, 0.021, 0.017]), centre(16, 6, 6, [0.011, -0.019, 0.023]), centre(24, 6, 6, [0.017, 0.013, -0.011]),
                    centre(36, 5, 6, [-0.021, 0.012, 0.019]), centre(30, 6, 5, [0.023, -0.014, 0.016])])
    radii = np.array([0.9, 1.1, 4.1, 3.1, 2.6], dtype=np.float32)
    rng = np.random.default_rng(7)
    return xyz, _expo(rng, 5, 1, radii), radii


def boxes_of_trips():
    return [(3, 3, 3), (5, 5, 5), (17, 12, 12), (13, 12, 12), (11, 11, 11)]


def cases():
    out = []
    for name in GEOMETRIES:
        for nt in (1, 3, 6):
            if nt == 1 or name in ("box", "skew", "rep"):
                out.append(("%s-%dterm-random" % (name, nt), name, "random", False) + atoms(name, nt))
    out.append(("rep-unique-random", "rep", "random", True) + atoms("rep", 1))
    out.append(("rep-unique-6term", "rep", "random", True) + atoms("rep", 6))
    out.append(("skew-unique-random", "skew", "random", True) + atoms("skew", 3))
    for kind in ("zero", "one", "spike"):
        out.append(("box-%s" % kind, "box", kind, False) + atoms("box", 3))
    out.append(("skew-spike", "skew", "spike", False) + atoms("skew", 1))
    out.append(("wide-trips", "wide", "random", False) + trips("wide"))
    out.append(("wide-trips-one", "wide", "one", False) + trips("wide"))
    return out


def find(tag):
    return [c for c in cases() if c[0] == tag][0]


def model_terms(xyz, expo, radii, seed=3):
    """Amplitudes in [0.5, 2] for the adjointness test (the same atoms through pdbeda_model_density)."""
    return np.random.default_rng(seed).uniform(0.5, 2.0, size=np.asarray(expo).shape)
