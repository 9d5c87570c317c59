"""The maps and cases of the resampling tests (shared by tests/test_resample_host.py and tests/test_gpu_resample.py): seeded, so both see the
same numbers.  The source geometries are ``box`` (a full periodic cell), ``skew`` (a cut-out of a skewed cell with permuted axes and a
start) and ``rep`` (a stored box larger than its cell) of tests/model_cases.py; a case is a dict ``name``, ``src``, ``dst`` (a DensityHeader),
``ops`` (n x 12), ``mean``, ``fill``, ``cutout`` (the case must leave a tenth of the destination uncovered) and maybe ``base`` / ``alpha``.

How the numbers are chosen.  The maps are white noise of unit variance, so nine voxels in ten exceed 0.1 in magnitude and so does an
interpolated value more often than not; the destinations are placed so that, by the checker alone, a quarter of every destination is
covered by such values and a tenth of every cut-out case is not covered at all (``guard``; tests/test_resample_host.py asserts it)."""
import io

import numpy as np

from pdb_eda_amd import ccp4, synthetic

import model_cases
import resample_checker

cellHeader = ccp4.cellHeader        # (looked up on import: without the feature neither test module loads)

TILE = (32, 4, 2)                   # RS_C, RS_R, RS_S of pdb_eda_amd/csrc/pdbeda_resample.h
LDS_VOX = 8192                      # RS_LDS_VOX
STAGED_ORDERS = (3,)                # the orders at which the kernel stages at all
MAX_OPS = 192                       # PDBEDA_RESAMPLE_MAX_OPS
SOURCES = ("box", "skew", "rep")
ORDERS = (0, 1, 3)
_grids, _cases = {}, None


def header_of(name):
    return model_cases.header_of(name)


def grid_of(name, seed=0):
    """White noise of unit variance on the geometry ``name``, float32 [ns][nr][nc]."""
    key = (name, seed)
    if key not in _grids:
        nc, nr, ns = (int(v) for v in header_of(name).ncrs)
        grid = np.random.default_rng(1000 + 17 * seed + sum(ord(ch) for ch in name)).standard_normal((ns, nr, nc)).astype(np.float32)
        grid.setflags(write=False)
        _grids[key] = grid
    return _grids[key]


def spec_header(**spec):
    """The header a CCP4 file of this MapSpec parses to."""
    s = synthetic.MapSpec(**spec)
    nc, nr, ns = s.ncrs
    return ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(s, np.zeros((ns, nr, nc), dtype=np.float32))))[0]


def centre_of(name):
    lo, hi = model_cases.box_of(name)
    return 0.5 * (lo + hi)


def rotation(rotvec):
    """Rodrigues' formula."""
    v = np.asarray(rotvec, dtype=np.float64)
    angle = float(np.linalg.norm(v))
    if angle == 0.0:
        return np.eye(3)
    k = v / angle
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K.dot(K)


def rigid(rotvec, about, shift):
    """x -> R (x - about) + about + shift as a (3, 4) operator."""
    rot, about = rotation(rotvec), np.asarray(about, dtype=np.float64)
    return np.hstack([rot, (about - rot.dot(about) + np.asarray(shift, dtype=np.float64)).reshape(3, 1)])


def grid_shift(header, steps):
    """The translation by ``steps`` grid steps along the crs axes of ``header``, as an operator."""
    frac = np.zeros(3)
    for crs_axis in range(3):
        xyz_axis = header.map2crs[crs_axis]
        frac[xyz_axis] = steps[crs_axis] / float(header.xyzInterval[xyz_axis])
    return np.hstack([np.eye(3), np.asarray(header.orthoMat, dtype=np.float64).dot(frac).reshape(3, 1)])


IDENTITY = ccp4.identityOperator()


def _case(name, src, dst, ops, mean=False, fill=0.0, cutout=False, **more):
    case = dict(name=name, src=src, dst=dst, ops=np.asarray(ops, dtype=np.float64).reshape(-1, 12), mean=mean, fill=np.float32(fill), cutout=cutout)
    case.update(more)
    return case


def window_header(name, lead, ncrs):
    """``name``'s cell and sampling with the stored box moved ``lead`` voxels before its own and ``ncrs`` voxels wide."""
    spec = dict(model_cases.SPECS[name])
    h = header_of(name)
    spec.setdefault("interval", tuple(int(v) for v in h.xyzInterval))
    spec.setdefault("cell", tuple(float(v) for v in h.xyzLength))
    spec.pop("spacing", None)
    start = spec.get("crs_start", (0, 0, 0))
    spec["crs_start"] = tuple(int(start[k]) - int(lead[k]) for k in range(3))
    spec["ncrs"] = tuple(int(v) for v in ncrs)
    return spec_header(**spec)


def many_ops(n, seed=5):
    """n small rigid motions about the middle of ``box`` (a periodic map serves every one of them)."""
    rng = np.random.default_rng(seed)
    about = centre_of("box")
    return np.array([rigid(rng.uniform(-0.3, 0.3, 3), about, rng.uniform(-1.0, 1.0, 3)) for _ in range(n)]).reshape(n, 12)


def cases():
    """Every case of the bit comparisons, by name."""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    for src in SOURCES:
        c = centre_of(src)
        # a general rotation plus shift onto a box of another spacing inside (or, periodic, around) the source
        half = (2.0, 1.0, 0.5) if src != "skew" else (0.9, 1.6, 0.5)
        out.append(_case("rotated-" + src, src, ccp4.boxHeader(c, half, 0.3), [rigid((0.05, -0.08, 0.12), c, (0.11, -0.07, 0.05))], cutout=False))
    c = centre_of("box")
    out.append(_case("finer", "box", ccp4.boxHeader(c, (2.5, 1.0, 0.6), 0.125), [rigid((0.2, -0.3, 0.4), c, (0.03, 0.02, -0.01))]))
    out.append(_case("coarser", "box", ccp4.boxHeader(c, (20.0, 8.0, 6.0), 2.0), [rigid((0.2, -0.3, 0.4), c, (0.3, 0.2, -0.1))]))
    shift = grid_shift(header_of("box"), (0.37, 0.21, 0.44))
    out.append(_case("one-tile", "box", spec_header(ncrs=TILE, interval=(64, 16, 8), spacing=0.5), [shift]))
    out.append(_case("past-tile", "box", spec_header(ncrs=tuple(v + 1 for v in TILE), interval=(64, 16, 8), spacing=0.5), [shift]))
    # first-valid on a cut-out: a window around skew's stored box; the second operator reaches source voxels for the columns before it
    skew = header_of("skew")
    window = window_header("skew", (4, 2, 1), (29, 13, 9))
    second = grid_shift(skew, (4.5, 0.25, 0.0))
    out.append(_case("cutout-nan", "skew", window, [IDENTITY, second], fill=np.nan, cutout=True))
    out.append(_case("cutout-negzero", "skew", window, [IDENTITY, second], fill=-0.0, cutout=True))
    out.append(_case("cutout-mean", "skew", window, [IDENTITY, second], mean=True, fill=-7.5, cutout=True))
    # mean mode on a periodic map: one, two and the most operators
    small = ccp4.boxHeader(c, (1.9, 0.5, 0.3), 0.25)
    for n in (1, 2, MAX_OPS):
        out.append(_case("mean-%d" % n, "box", small, many_ops(n), mean=True))
    # base + alpha * value: everything covered (periodic) and a cut-out
    rot_box = out[0]
    nc, nr, ns = (int(v) for v in rot_box["dst"].ncrs)
    base = np.random.default_rng(77).standard_normal((ns, nr, nc)).astype(np.float32)
    out.append(_case("base-box", "box", rot_box["dst"], rot_box["ops"], base=base, alpha=-0.625))
    nc, nr, ns = (int(v) for v in window.ncrs)
    base = np.random.default_rng(78).standard_normal((ns, nr, nc)).astype(np.float32)
    out.append(_case("base-cutout", "skew", window, [IDENTITY, second], fill=np.nan, cutout=True, base=base, alpha=1.75))
    # staging (order 3): a coarser destination whose full tiles have a footprint just inside the LDS budget, and one just outside it
    frac_shift = grid_shift(header_of("box"), (0.13, 0.21, 0.17))
    out.append(_case("budget-inside", "box", spec_header(ncrs=(40, 6, 3), interval=(80, 12, 6), cell=(80.0, 12.0, 6.0)), [frac_shift]))
    out.append(_case("budget-outside", "box", spec_header(ncrs=(40, 6, 3), interval=(80, 12, 6), cell=(80.0, 15.0, 6.0)), [frac_shift]))
    _cases = dict((case["name"], case) for case in out)
    return _cases


_wanted = {}


def wanted(name, order):
    """The checker's (out, count) of a case, computed once and shared (never modified)."""
    key = (name, order)
    if key not in _wanted:
        case = cases()[name]
        out, count = resample_checker.resample(header_of(case["src"]), grid_of(case["src"]), case["dst"], case["ops"], order, case["mean"], case["fill"], case.get("base"),
                                               case.get("alpha", 1.0))
        out.setflags(write=False)
        count.setflags(write=False)
        _wanted[key] = (out, count)
    return _wanted[key]


def guard(name, order):
    """(fraction of the destination that is covered AND holds a magnitude above 0.1, fraction that is not covered), by the checker alone."""
    out, count = wanted(name, order)
    with np.errstate(invalid="ignore"):
        strong = (count > 0) & (np.abs(out) > 0.1)
    return float(strong.mean()), float((count == 0).mean())


def staged_pairs(case, order, grown=True):
    """The (tile, operator) pairs the kernel serves from LDS when no workgroup leaves its operator loop early: at a staged order, those
    whose box fits the budget."""
    return int((tile_footprints(case, order, grown) <= LDS_VOX).sum()) if order in STAGED_ORDERS else 0


def tile_footprints(case, order, grown=True):
    """Per (tile, operator): the number of source voxels in the box the kernel stages -- the tile's eight corners under the operator, floor
    and ceil of their grid positions, grown by the support and one voxel of safety.  [n_tiles][n_ops] int64, tiles in launch order."""
    src, dst = header_of(case["src"]), case["dst"]
    lo_grow, hi_grow = {0: (1, 1), 1: (1, 2), 3: (2, 3)}[order] if grown else (0, 0)
    n = [int(v) for v in dst.ncrs]
    tiles = [(n[k] + TILE[k] - 1) // TILE[k] for k in range(3)]
    out = []
    for ts in range(tiles[2]):
        for tr in range(tiles[1]):
            for tc in range(tiles[0]):
                c0 = [tc * TILE[0], tr * TILE[1], ts * TILE[2]]
                c1 = [min(c0[k] + TILE[k], n[k]) - 1 for k in range(3)]
                corners = np.array([[(c1 if j & 1 else c0)[0], (c1 if j & 2 else c0)[1], (c1 if j & 4 else c0)[2]] for j in range(8)])
                p = resample_checker.crs2xyz(dst, corners)
                row = []
                for op in case["ops"]:
                    f = resample_checker.xyz2frac(src, resample_checker.apply_operator(op, p))
                    dims = (np.ceil(f.max(axis=0)) + hi_grow) - (np.floor(f.min(axis=0)) - lo_grow) + 1
                    row.append(int(dims[0]) * int(dims[1]) * int(dims[2]))
                out.append(row)
    return np.array(out, dtype=np.int64)


# ---- two synthetic entries of one molecule: the second moved by a known rigid motion, put on another grid, with two planted sites ----
PAIR_SIGMA = 0.9            # A: the width of every Gaussian atom (the grids sample it at 0.5 and 0.4 A)
PAIR_PLANTED_AMP = 1.5      # the planted sites against atoms of amplitude 1
_pair = None


def _gaussians(header, centres, amps):
    nc, nr, ns = (int(v) for v in header.ncrs)
    xyz = header.crs2xyz_array(resample_checker.all_crs(header))
    rho = np.zeros(len(xyz))
    for centre, amp in zip(centres, amps):
        rho += amp * np.exp(-0.5 * ((xyz - centre) ** 2).sum(axis=1) / PAIR_SIGMA ** 2)
    return rho.astype(np.float32).reshape(ns, nr, nc)


def entry_pair():
    """A dict: ``first`` / ``second`` = (header, grid, CA coordinates), ``motion`` (first frame -> second frame), ``planted`` (the two sites
    of the second entry, in the FIRST frame)."""
    global _pair
    if _pair is None:
        rng = np.random.default_rng(2024)
        h1 = spec_header(ncrs=(40, 36, 32), interval=(60, 54, 48), crs_start=(-5, 3, 2), spacing=0.5)
        c1 = np.array(h1.crs2xyzCoord([19.5, 17.5, 15.5]), dtype=np.float64)
        atoms1 = c1 + rng.uniform(-4.0, 4.0, size=(40, 3))
        planted1 = c1 + np.array([[5.5, -4.5, 4.0], [-5.0, 5.0, -4.5]])
        motion = rigid((0.3, -0.2, 0.5), c1, (7.3, -2.1, 4.4))
        h2 = spec_header(ncrs=(56, 50, 46), interval=(80, 70, 64), crs_start=(3, -9, 7), spacing=0.4)
        c2 = np.array(h2.crs2xyzCoord([27.5, 24.5, 22.5]), dtype=np.float64)
        motion[:, 3] += c2 - ccp4.applyOperator(motion, c1[None, :])[0]          # the molecule sits in the middle of the second box
        atoms2 = ccp4.applyOperator(motion, atoms1)
        planted2 = ccp4.applyOperator(motion, planted1)
        g1 = _gaussians(h1, atoms1, np.ones(len(atoms1)))
        g2 = _gaussians(h2, np.concatenate([atoms2, planted2]), np.concatenate([np.ones(len(atoms2)), np.full(len(planted2), PAIR_PLANTED_AMP)]))
        _pair = dict(first=(h1, g1, atoms1), second=(h2, g2, atoms2), motion=motion, planted=planted1)
    return _pair
