"""Inputs of the crystal-contact edge tests (tests/test_contacts_host.py proves on the CPU that each reaches the corner it is named for,
tests/test_gpu_contacts_edges.py runs them on the device), as functions of a seed, and a plain-Python restatement of the host's grid rule
(make_cell_grid / query_grid in pdb_eda_amd/csrc/pdbeda_cellgrid.h; tests/test_cellgrid_host.py holds the planner itself against it).
The restatement only proves that a case reaches its corner; an expected result always comes from tests/contacts_checker.py."""
import functools
import itertools
import math

import numpy as np

import contacts_checker as chk

PINNED_BLOCK = 4 << 20          # PINNED_BLOCK_BYTES (pdbeda_stage.h), the context's pinned block: what pinned_out hands out per call
SCAN_TILE = 8 * 1024            # k_grid_scan: 1024 lanes x 8 cells per trip
MAX_SHIFT = 1 << 20             # check_images: the largest cell shift


# ---- the grid rule ------------------------------------------------------------------------------------------------------------------------
def cell_grid(lo, hi, cutoff, n_points):
    """make_cell_grid: (edge, dims, n_cells, coarsening steps), or None where it refuses -- an extent that is negative or not finite.  The same
    operations in the same order, in Python floats (fp64)."""
    extents = [float(hi[q]) - float(lo[q]) for q in range(3)]
    if not all(e >= 0.0 and math.isfinite(e) for e in extents):
        return None
    cap = float(min(1 << 22, max(4096, 8 * int(n_points))))
    edge = float(cutoff) * (1.0 + 1e-6)
    steps = 0
    while True:
        cells = 1.0
        for q in range(3):
            cells *= math.floor((float(hi[q]) - float(lo[q])) / edge) + 1.0
        if cells <= cap:
            break
        edge *= 1.25
        steps += 1
    dims = tuple(int(math.floor((float(hi[q]) - float(lo[q])) / edge)) + 1 for q in range(3))
    return edge, dims, dims[0] * dims[1] * dims[2], steps


def query_grid(q, cutoff, n_points):
    """query_grid: the grid over the queries' bounding box grown by twice the cutoff."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    lo = [float(v) - 2 * float(cutoff) for v in q.min(axis=0)]
    hi = [float(v) + 2 * float(cutoff) for v in q.max(axis=0)]
    return cell_grid(lo, hi, cutoff, n_points)


def cell_of(q, cutoff, n_points, xyz):
    """grid_cell of every xyz row in query_grid(q): the cell number (cz * dim[1] + cy) * dim[0] + cx, clamped to the grid as the device clamps."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    edge, dims, _, _ = query_grid(q, cutoff, n_points)
    lo = q.min(axis=0) - 2 * float(cutoff)
    c = np.floor((np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - lo) / edge)
    c = np.clip(c, 0, np.array(dims) - 1).astype(np.int64)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def nearest_point(q, p, rows):
    """Index of the nearest p for the listed queries (the checker's distance formula; first index on ties)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    return np.array([int(np.argmin(chk.pair_dist(q[i][None, :], p))) for i in rows], dtype=np.int64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- 1. large results -----------------------------------------------------------------------------------------------------------------------
def mixed_path(seed=0):
    """(q, p, cutoff): 300 000 queries against 230 000 points, uniform in a 200 A cube at 3 decimals."""
    rng = np.random.default_rng(1000 + seed)
    q = np.round(rng.uniform(0.0, 200.0, (300000, 3)), 3)
    p = np.round(rng.uniform(0.0, 200.0, (230000, 3)), 3)
    return q, p, 1.0


def device_path(seed=0):
    """(q, p, cutoff): 600 000 queries against 1 000 points in a 60 A cube."""
    rng = np.random.default_rng(1100 + seed)
    q = np.round(rng.uniform(0.0, 60.0, (600000, 3)), 3)
    p = np.round(rng.uniform(0.0, 60.0, (1000, 3)), 3)
    return q, p, 1.5


DIAG_CELL = (40.0, 46.0, 52.0)


def identity_ops():
    return np.hstack([np.eye(3), np.zeros((3, 1))])[None, :, :]


def many_candidates(seed=0):
    """(query, poly, rot, ortho, cand, cutoff): two atoms, the identity operator, every shift of [-51, 51]^3 but 0: 103^3 - 1 = 1 092 726
    candidates, whose keep flags (4 bytes each) exceed the pinned block."""
    poly = np.array([[1.0, 2.0, 3.0], [30.0, 40.0, 20.0]])
    rng = np.random.default_rng(1200 + seed)
    query = np.round(np.concatenate([poly[[0, 1, 0]] + rng.uniform(-3.0, 3.0, (3, 3)), poly[[1]] + [40.0, 0.0, 0.5], poly[[0]] + [0.0, -46.0, 0.25]]), 3)
    r = np.arange(-51, 52)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    n = n[np.any(n != 0, axis=1)]
    cand = np.hstack([np.zeros((len(n), 1), dtype=np.int64), n]).astype(np.int32)
    return query, poly, identity_ops(), np.diag(DIAG_CELL), cand, 45.0


def many_images(seed=0):
    """(poly, rot, ortho, cand): 40 images of 5 000 atoms in P 21 21 21: 200 000 points, 4.8 MB."""
    ortho = chk.ortho_matrix(chk.CELLS["P212121"][0], chk.CELLS["P212121"][1])
    rot = chk.smtry("P212121", ortho)
    poly = chk.blob(5000, 1300 + seed, -3.0, 36.0)
    cand = np.array([(op,) + n for op in range(4) for n in itertools.product((-1, 0, 1), repeat=3) if (op, n) != (0, (0, 0, 0))][:40], dtype=np.int32)
    return poly, rot, ortho, cand


# ---- 2, 3, 9: the ordinary crystal the switch, capacity and poison tests share ----------------------------------------------------------------
def ordinary_coord(seed=0):
    """(q, p, cutoff): 3 000 queries, 5 000 points, about half of the queries with a contact."""
    rng = np.random.default_rng(2000 + seed)
    return np.round(rng.uniform(-20, 20, (3000, 3)), 3), np.round(rng.uniform(-25, 25, (5000, 3)), 3), 1.7


def ordinary_crystal(seed=0):
    """(query, poly, rot, ortho, cand, cutoff): P 61, 1 200 atoms and 200 ligand queries beside them."""
    from pdb_eda_amd import crystalContacts
    rot, ortho, poly = chk.crystal("P61", n_atoms=1200, seed=2100 + seed)
    rng = np.random.default_rng(2200 + seed)
    query = np.concatenate([poly, np.round(rng.uniform(-6.0, 40.0, (200, 3)), 3)])
    return query, poly, rot, ortho, crystalContacts.candidateImages(rot, ortho, poly, 2.5), 2.5


# ---- 4. degenerate sets -------------------------------------------------------------------------------------------------------------------------
def degenerate_coord(seed=0):
    """{name: (q, p, cutoff)}."""
    rng = np.random.default_rng(4000 + seed)
    out = {}
    out["one on one"] = (np.array([[1.0, 2.0, 3.0]]), np.array([[1.0, 2.0, 3.0]]), 5.0)
    above = float(np.nextafter(5.0, np.inf))
    for axis, sign in itertools.product(range(3), (1.0, -1.0)):
        for tag, r in (("at", 5.0), ("past", above)):
            p = np.zeros((1, 3))
            p[0, axis] = sign * r
            out["%s cutoff %s%s" % (tag, "+-"[sign < 0], "xyz"[axis])] = (np.zeros((1, 3)), p, 5.0)
    out["at cutoff 3 4 0"] = (np.zeros((1, 3)), np.array([[3.0, 4.0, 0.0]]), 5.0)
    out["past cutoff 3 4 0"] = (np.zeros((1, 3)), np.array([[3.0, float(np.nextafter(4.0, np.inf)), 0.0]]), 5.0)
    out["below cutoff 3 4 0"] = (np.zeros((1, 3)), np.array([[3.0, 4.0, 0.0]]), float(np.nextafter(5.0, 0.0)))
    out["signed zeros"] = (np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [1.0, -0.0, 0.0], [-0.0, 1.5, 0.0]]), np.array([[-0.0, 0.0, -0.0]]), 1.0)
    t = np.round(np.sort(rng.uniform(0.0, 900.0, 2000)), 3)
    u = np.round(np.sort(rng.uniform(-1.0, 901.0, 2000)), 3)
    out["collinear on an axis"] = (np.stack([t, np.full(2000, 7.0), np.full(2000, -3.0)], axis=1), np.stack([u, np.full(2000, 7.0), np.full(2000, -3.0)], axis=1), 0.25)
    d = np.array([1.0, 2.0, -3.0])
    out["collinear on a diagonal"] = (np.round(t / 4.0, 3)[:, None] * d, np.round(u / 4.0, 3)[:, None] * d, 0.25)
    out["coplanar"] = (np.hstack([np.round(rng.uniform(0.0, 60.0, (2000, 2)), 3), np.full((2000, 1), 5.0)]),
                       np.hstack([np.round(rng.uniform(-1.0, 61.0, (2000, 2)), 3), np.full((2000, 1), 5.0)]), 1.0)
    c = np.array([10.5, -3.25, 7.125])
    out["one crowded cell"] = (np.round(c + rng.normal(0.0, 1.0, (300, 3)), 3), np.tile(c, (5000, 1)), 1.5)
    q, p, cutoff = ordinary_coord(seed)
    for shift in (9000.0, 1e6):
        out["shifted by %g" % shift] = (q + shift, p + shift, cutoff)
    return out


def degenerate_crystal(seed=0):
    """{name: (query, poly, rot, ortho, cand, cutoff)}: polymers whose own grid gp is degenerate."""
    from pdb_eda_amd import crystalContacts
    rng = np.random.default_rng(4500 + seed)
    ortho = np.diag(DIAG_CELL)
    rot = np.array(chk.smtry("P212121", ortho))
    shifts = np.array([(op,) + n for op in range(4) for n in itertools.product((-2, -1, 0, 1, 2), repeat=3) if (op, n) != (0, (0, 0, 0))], dtype=np.int32)
    out = {}
    one = np.array([[1.0, 2.0, 3.0]])

    def near(poly):          # (queries around the first 40 atoms and all over the neighbouring cells)
        return np.round(np.concatenate([poly[:40] + rng.uniform(-30.0, 30.0, (min(len(poly), 40), 3)), rng.uniform(-60.0, 60.0, (150, 3))]), 3)

    out["one atom"] = (np.concatenate([one, near(one)]), one, rot, ortho, shifts, 47.0)
    same = np.tile(one, (50, 1))
    out["coincident atoms"] = (np.concatenate([same[:2], near(same)]), same, rot, ortho, shifts, 47.0)
    line = np.stack([np.round(np.linspace(0.0, 39.0, 80), 3), np.full(80, 10.0), np.full(80, 10.0)], axis=1)
    out["collinear atoms"] = (np.concatenate([line, near(line)]), line, rot, ortho, crystalContacts.candidateImages(rot, ortho, line, 8.0), 8.0)
    return out


# ---- 5. grid corners --------------------------------------------------------------------------------------------------------------------------
def _corner_box(rng, extents, n_q, n_p, cutoff, every=2, most=None):
    """Two corner queries and random ones, a share of them within a cutoff of a face; points all over the crop box (the queries' box grown
    by twice the cutoff: the first and the last cell of every axis hold points), and one point within the cutoff of every ``every``-th query
    (``most`` of them at the most)."""
    ext = np.asarray(extents, dtype=np.float64)
    q = rng.uniform(0.0, 1.0, (n_q, 3)) * ext
    face = rng.integers(0, 6, n_q // 2)
    for i, f in enumerate(face):           # (pushed to within a cutoff of face f)
        q[i, f % 3] = rng.uniform(0.0, cutoff) if f < 3 else ext[f % 3] - rng.uniform(0.0, cutoff)
    q = np.round(q, 3)
    q[0], q[1] = 0.0, ext
    step = rng.normal(0.0, 1.0, (len(q[::every][:most]), 3))
    step *= (rng.uniform(0.1, 0.95, len(step)) * cutoff / np.sqrt((step * step).sum(axis=1)))[:, None]
    partners = np.round(q[::every][:most] + step, 3)
    fill = np.round(rng.uniform(0.0, 1.0, (n_p - len(partners), 3)) * (ext + 4.0 * cutoff) - 2.0 * cutoff, 3)
    return q, np.concatenate([partners, fill])


# name: (extents of the queries' box, queries, points, cells wanted).  At cutoff 1 the box grows by 4 per axis and the edge is 1.000001, so the
# dims are the extents + 4.  The last cell of an axis begins more than a cutoff beyond every query, so in the 8 200-cell grid the eight cells
# past the first scan tile (the far end of the last row of the last layer) can hold no contact; the 9 800-cell grid has eight whole layers
# past the tile, seven of them within reach of a query.
GRID_CORNERS = {
    "one tile": ((28.0, 12.0, 12.0), 600, 1500, 8192),
    "one tile and eight cells": ((4.0, 21.0, 37.0), 600, 1500, 8200),
    "one tile and eight z layers": ((4.0, 21.0, 45.0), 600, 1500, 9800),
    "two tiles": ((28.0, 28.0, 12.0), 1000, 2500, 16384),
}


def grid_corners(seed=0):
    """{name: (q, p, cutoff)}: the four tile cases, the cap's lower bound, and the edge that coarsens more than 20 times."""
    rng = np.random.default_rng(5000 + seed)
    out = {}
    for name, (ext, n_q, n_p, _) in GRID_CORNERS.items():
        out[name] = _corner_box(rng, ext, n_q, n_p, 1.0) + (1.0,)
    out["lower bound of the cap"] = _corner_box(rng, (30.0, 30.0, 30.0), 290, 215, 1.0, every=1, most=205) + (1.0,)
    anchors = np.array([[0.0, 0.0, 0.0], [10000.0, 0.0, 0.0], [0.0, 9000.0, 0.0]])
    q = np.concatenate([anchors] + [np.round(a + rng.uniform(-3.0, 3.0, (100, 3)), 3) for a in anchors])
    step = rng.normal(0.0, 1.0, (len(q), 3))
    step *= (rng.uniform(0.1, 0.9, len(q)) * 0.5 / np.sqrt((step * step).sum(axis=1)))[:, None]
    p = np.concatenate([np.round(q + step, 3)[:250]] + [np.round(a + rng.uniform(-4.0, 4.0, (120, 3)), 3) for a in anchors])
    out["far clusters"] = (q, p, 0.5)
    return out


# ---- 6. exact-boundary images ------------------------------------------------------------------------------------------------------------------
def boundary_identity(seed=0):
    """(poly, rot, ortho, cand): (35, 10, 10) - (40, 0, 0) lies exactly 5 from (0, 10, 10); no other atom comes within 5 of an image."""
    from pdb_eda_amd import crystalContacts
    rng = np.random.default_rng(6000 + seed)
    fill = np.round(np.stack([rng.uniform(1.0, 34.0, 500), rng.uniform(0.0, 30.0, 500), rng.uniform(0.0, 30.0, 500)], axis=1), 3)
    poly = np.concatenate([[[0.0, 10.0, 10.0], [35.0, 10.0, 10.0]], fill])
    rot, ortho = identity_ops(), np.diag(DIAG_CELL)
    return poly, rot, ortho, crystalContacts.candidateImages(rot, ortho, poly, 5.0)


def boundary_twofold(seed=0):
    """(poly, rot, ortho, cand): the identity and the two-fold screw (x + 20, -y, -z) (exact in binary).  The fill keeps y in [6, 17] and
    z in [6, 20], so its rotated copies stay more than 8 A away whatever the shift; (10, 2.5, 0) maps to (30, -2.5, 0), exactly 5 from (30, 2.5, 0), and with n = (-1, 0, 0) the latter maps
    to (10, -2.5, 0), exactly 5 from the former."""
    from pdb_eda_amd import crystalContacts
    rng = np.random.default_rng(6100 + seed)
    fill = np.round(np.stack([rng.uniform(1.0, 34.0, 500), rng.uniform(6.0, 17.0, 500), rng.uniform(6.0, 20.0, 500)], axis=1), 3)
    poly = np.concatenate([[[0.0, 10.0, 10.0], [35.0, 10.0, 10.0], [10.0, 2.5, 0.0], [30.0, 2.5, 0.0]], fill])
    screw = np.array([[1.0, 0.0, 0.0, 20.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]])
    rot, ortho = np.stack([identity_ops()[0], screw]), np.diag(DIAG_CELL)
    return poly, rot, ortho, crystalContacts.candidateImages(rot, ortho, poly, 5.0)


BELOW_FIVE = float(np.nextafter(5.0, 0.0))


# ---- 8. branches ----------------------------------------------------------------------------------------------------------------------------
def far_queries(seed=0):
    """The ordinary crystal with queries 1 000 A away from it: images are kept, every image atom is cropped from the queries' grid."""
    query, poly, rot, ortho, cand, cutoff = ordinary_crystal(seed)
    return query[-200:] + 1000.0, poly, rot, ortho, cand, cutoff


# ---- expected results, computed once per process ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_coord(family, name=None, seed=0):
    """The checker's (index, distance) of a coord_contacts case; the KD checker where the brute one is not affordable."""
    q, p, cutoff = coord_case(family, name, seed)
    return _frozen(*chk.coord_contacts(q, p, cutoff, kd=len(q) * len(p) > 4e7))


@functools.lru_cache(maxsize=None)
def coord_case(family, name=None, seed=0):
    case = {"mixed": mixed_path, "device": device_path, "ordinary": ordinary_coord}[family](seed) if name is None else \
        {"degenerate": degenerate_coord, "corners": grid_corners}[family](seed)[name]
    _frozen(case[0], case[1])
    return case


@functools.lru_cache(maxsize=None)
def crystal_case(family, name=None, seed=0):
    case = {"ordinary": ordinary_crystal, "far": far_queries}[family](seed) if name is None else degenerate_crystal(seed)[name]
    return tuple(np.asarray(v) if i < 5 else v for i, v in enumerate(case))


@functools.lru_cache(maxsize=None)
def expected_crystal(family, name=None, seed=0):
    """The checker's (keep flags, index, distance) of a crystal_contacts case."""
    query, poly, rot, ortho, cand, cutoff = crystal_case(family, name, seed)
    return _frozen(*chk.crystal_contacts(query, rot, ortho, poly, cand, cutoff))
