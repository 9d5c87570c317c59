"""The maps, tables and seeds of the spread tests (shared by tests/test_spread_host.py, tests/test_spread_plan_host.py and
tests/test_gpu_spread.py): seeded, so all see the same numbers.  The geometries box, skew and rep are those of tests/model_cases.py; the others
exist for the kernel's work units.  ``compared_cases()`` is the list the GPU test holds to the checker's bits and the host test guards:
every case that is not "none" or "all" must leave a good part of the map reached AND a good part unreached, or it shows nothing."""
import io

import numpy as np

from pdb_eda_amd import ccp4, synthetic

import model_cases

TILE = (64, 8, 8)           # SP_TILE_C, SP_TILE_R, SP_TILE_S of pdb_eda_amd/csrc/pdbeda_spreadplan.h
MAX_OFFSETS, MAX_REACH = 16384, 32
spreadTable = ccp4.spreadTable          # (looked up on import: without the feature no test module of the spread loads)

SPECS = dict((name, model_cases.SPECS[name]) for name in ("box", "skew", "rep"))
SPECS.update({
    "tile": dict(ncrs=TILE, spacing=0.5),                                                   # exactly one output tile
    "tile_past": dict(ncrs=(TILE[0] + 1, TILE[1] + 1, TILE[2] + 1), spacing=0.5),           # one voxel more on every axis
    "two": dict(ncrs=(2 * TILE[0], 2 * TILE[1], 2 * TILE[2]), spacing=0.5),                 # two tiles on every axis
    "line": dict(ncrs=(70, 1, 1), spacing=0.5),                                             # periodic: a reach of 32 meets itself
    "cut": dict(ncrs=(70, 1, 1), interval=(100, 1, 1), spacing=0.5),                        # the same line in a 100-step cell
    "thin": dict(ncrs=(21, 9, 3), spacing=0.5),                                             # a periodic axis of 3 under a reach of 5: wraps more than once
    "big": dict(ncrs=(40, 36, 32), spacing=0.5),                                            # for the largest ball
})
_headers, _cache = {}, {}


def spec_of(name):
    return synthetic.MapSpec(**SPECS[name])


def header_of(name):
    if name not in _headers:
        spec = spec_of(name)
        nc, nr, ns = spec.ncrs
        _headers[name] = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((ns, nr, nc), dtype=np.float32))))[0]
    return _headers[name]


def intervals_of(name):
    return [int(v) for v in header_of(name).crsInterval]


def shape_of(name):
    nc, nr, ns = spec_of(name).ncrs
    return ns, nr, nc


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def largest_ball(name="big"):
    """The largest ball of spreadTable (in steps of 0.05 A) that stays within MAX_OFFSETS: (offsets, distance, radius)."""
    key = ("largest", name)
    if key not in _cache:
        radius = 8.5
        while True:
            try:
                offsets, distance = spreadTable(header_of(name), radius)
                break
            except ValueError:
                radius = round(radius - 0.05, 2)
        _cache[key] = (offsets, distance, radius)
    return _cache[key]


def needle():
    """(k, 0, 0) for |k| <= 32 in the order of |k|, -k before +k: the ranks along dc fall to 0 and rise, one eligible row of the largest reach."""
    ks = [0] + [s * k for k in range(1, MAX_REACH + 1) for s in (-1, 1)]
    return np.array([[k, 0, 0] for k in ks], dtype=np.int32)


def needles3():
    """Needles along all three axes in the order of |k|: the largest reach on every axis, so the smallest tile with the largest staged box."""
    out = [[0, 0, 0]]
    for k in range(1, MAX_REACH + 1):
        for axis in range(3):
            for s in (-1, 1):
                o = [0, 0, 0]
                o[axis] = s * k
                out.append(o)
    return np.array(out, dtype=np.int32)


def needle_up():
    """(k, 0, 0) for k = -32 .. 32 in that order: one rising row of 65 offsets, more than a 64-bit window holds behind its minimum."""
    return np.array([[k, 0, 0] for k in range(-MAX_REACH, MAX_REACH + 1)], dtype=np.int32)


def table(name, geometry):
    """name -> (offsets int32 (n, 3), row-compilable?).  Ball tables are the geometry's own."""
    key = ("table", name, geometry)
    if key in _cache:
        return _cache[key]
    h = header_of(geometry)
    if name == "ball10":
        out = (spreadTable(h, 1.0)[0], True)
    elif name == "ball25":
        out = (spreadTable(h, 2.5)[0], True)
    elif name == "single":
        out = (np.zeros((1, 3), dtype=np.int32), True)
    elif name == "needle":
        out = (needle(), True)
    elif name == "needles3":
        out = (needles3(), True)
    elif name == "needle_up":
        out = (needle_up(), False)
    elif name == "largest":
        out = (largest_ball(geometry)[0], True)
    elif name == "shuffled":
        o = spreadTable(h, 2.5)[0]
        out = (o[np.random.default_rng(5).permutation(len(o))], False)
    elif name == "holed":                                    # the ball without its second shell (the nearest neighbours): the rows through the middle have gaps
        o, d = spreadTable(h, 2.5)
        shell = np.unique(d)[1]
        out = (o[d != shell], False)
    elif name == "duplicate":                                # offset 3 once more, at the end
        o = spreadTable(h, 2.5)[0]
        out = (np.concatenate([o, o[3:4]]), False)
    else:
        raise KeyError(name)
    out[0].setflags(write=False)
    _cache[key] = out
    return out


TABLES = ("ball10", "ball25", "single", "needle", "needles3", "needle_up", "shuffled", "holed", "duplicate")


# ---- seeds ------------------------------------------------------------------------------------------------------------------------------
def noise(geometry, seed=0):
    key = ("noise", geometry, seed)
    if key not in _cache:
        g = synthetic.smooth_noise(shape_of(geometry), 300 + seed, 1.0).astype(np.float64)
        g = np.ascontiguousarray(g / max(float(g.std()), 1e-6), dtype=np.float32)
        g.setflags(write=False)
        _cache[key] = g
    return _cache[key]


def grid(kind, geometry):
    """kind -> (float32 grid [s][r][c], threshold, below)."""
    shape = shape_of(geometry)
    ns, nr, nc = shape
    x = np.zeros(shape, dtype=np.float32)
    if kind == "one":
        x[ns // 2, nr // 2, nc // 3] = 1.0
        return x, 0.5, False
    if kind == "pair":                                       # two seeds, the voxel between them equidistant from both: the table's order decides
        x[ns // 2, nr // 2, nc // 3 - 2] = 1.0
        x[ns // 2, nr // 2, nc // 3 + 2] = 2.0
        return x, 0.5, False
    if kind == "none":
        return x, 0.5, False
    if kind == "all":
        return x + np.float32(1.0), 0.5, False
    if kind == "blobs":                                      # half the map in blobs a few voxels across: an erosion leaves something
        key = ("blobs", geometry)
        if key not in _cache:
            b = synthetic.smooth_noise(shape, 300, 3.0).astype(np.float64)
            _cache[key] = np.ascontiguousarray(b / max(float(b.std()), 1e-6), dtype=np.float32)
            _cache[key].setflags(write=False)
        return _cache[key], float(np.quantile(_cache[key], 0.5)), False
    g = noise(geometry)
    if kind.startswith("noise"):                             # noiseNN: the NN / 10 per cent highest voxels are seeds
        return g, float(np.quantile(g, 1.0 - 0.001 * int(kind[5:]))), False
    if kind.startswith("below"):                             # belowNN: the NN / 10 per cent lowest, under PDBEDA_SPREAD_BELOW
        return g, float(np.quantile(g, 0.001 * int(kind[5:]))), True
    if kind in ("special", "special_below"):                 # sparse seeds, and voxels that are not finite: a NaN is never one, an infinity on its side is
        x = g.copy()
        flat = x.reshape(-1)
        n = flat.size
        flat[n // 7] = np.nan
        flat[n // 5] = np.inf
        flat[n // 3] = -np.inf
        flat[n // 2] = np.nan
        below = kind == "special_below"
        return x, float(np.quantile(g, 0.01 if below else 0.99)), below
    raise KeyError(kind)


def base_of(geometry):
    """A base map with a NaN, a -0.0, an infinity and values of both signs."""
    b = (noise(geometry, 1).astype(np.float64) * 3.0 + 0.5).astype(np.float32)
    flat = b.reshape(-1)
    flat[1] = np.nan
    flat[2] = -0.0
    flat[3] = np.inf
    flat[flat.size // 2] = -0.0
    return b


def atoms(geometry, n=14, seed=23):
    """(xyz float64 (n, 3), radii float32) of atoms inside and just outside the stored box, radii 0.6 .. 1.4 A."""
    rng = np.random.default_rng(seed)
    lo, hi = model_cases.box_of(geometry)
    xyz = rng.uniform(lo - 0.5, hi + 0.5, size=(n, 3))
    return xyz, rng.uniform(0.6, 1.4, size=n).astype(np.float32)


def values_of(n, kind="rank"):
    """The values of a table of n offsets: 'rank' -- values[t] = t, so the ranks themselves are compared; 'odd' -- values that are not finite and
    a payload NaN among them, whose bits must be kept."""
    v = np.arange(n + 1, dtype=np.float32)
    if kind == "odd":
        v = v * np.float32(0.37) - np.float32(1.5)
        v[0] = -0.0
        v[n] = np.inf
        if n > 2:
            v[1] = np.array([0x7fc12345], dtype=np.uint32).view(np.float32)[0]
            v[2] = -np.inf
    return v


def compared_cases():
    """(tag, geometry, table, seeds, with base?, values kind).  Sparse seeds for the wide tables: the box noise at a cut of 2.6 sigma under a
    reach of 2.5 A reaches every voxel."""
    out = []
    for geometry in ("box", "skew", "rep"):
        out += [(geometry, "ball10", "noise30", False, "rank"), (geometry, "ball25", "one", False, "rank"), (geometry, "ball25", "pair", True, "rank"),
                (geometry, "single", "noise300", False, "odd"), (geometry, "ball10", "below30", True, "odd")]
    out += [("box", "needle", "noise10", False, "rank"), ("box", "needles3", "noise10", False, "rank"), ("box", "needle_up", "noise10", False, "rank"),
            ("box", "shuffled", "one", False, "rank"), ("box", "holed", "pair", False, "rank"), ("box", "duplicate", "one", True, "odd"),
            ("box", "ball10", "special", True, "rank"), ("box", "ball10", "special_below", False, "rank"),
            ("box", "ball25", "none", True, "odd"), ("box", "ball25", "all", False, "rank"),
            ("skew", "shuffled", "pair", False, "rank"),
            ("tile", "ball25", "noise2", False, "rank"), ("tile_past", "ball25", "noise2", True, "rank"), ("two", "ball25", "noise2", False, "rank"),
            ("tile_past", "needles3", "noise2", False, "rank"), ("two", "holed", "noise2", False, "rank"),
            ("line", "needle", "one", False, "rank"), ("cut", "needle", "one", False, "rank"), ("line", "needle_up", "one", False, "rank"),
            ("thin", "ball25", "one", False, "rank"), ("thin", "ball25", "below30", False, "rank")]
    return [("%s-%s-%s%s" % (g, t, s, "-base" if b else ""), g, t, s, b, v) for g, t, s, b, v in out]
