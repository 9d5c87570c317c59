"""Seeded inputs of tests/test_cloud_host.py and tests/test_gpu_cloud.py: flattened ``pdbeda_cloud_atoms`` entries (no Structure
objects) on three kinds of map.

big_entry()      one 224^3 map at 0.5 A with the whole cell stored and 48 000 atom sites on a jittered lattice: prefixes of it are
                 entries on either side of the three sizes at which pdbeda_aggregate_cloud changes its path (tests/test_cloud_host.py: switch_points()).
world_entry()    the first 400 positions of tests/batch_limit_cases.py (they start 4 voxels outside the stored box) on that world's
                 smooth map, or on unit white noise with 3 A spheres (about ten clouds an atom); residues of 8 positions, which lie
                 far apart except every fourth and the one before it: rows from 12 electrons (two atoms) on.
crafted()        a 40^3 orthogonal map painted voxel by voxel with small dyadic densities, and a handful of atoms on voxel centres
                 per decision rule.

An entry is a dict: the nine arrays of DeviceMap.aggregate_cloud (``ARGS``), ``cutoff`` (the density cut-off, float32) and
``min_electrons``."""
import io

import numpy as np

import batch_limit_cases

ARGS = ("xyz", "radius", "weight", "residue", "alias", "key", "bonded_off", "bonded", "owner_key")


def header_of(spec):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(spec))


def call(m, e):
    """m.aggregate_cloud (a DeviceMap, or the oracle) on entry e."""
    return m.aggregate_cloud(*[e[k] for k in ARGS], e["cutoff"], e["min_electrons"])


def last_of_coordinate(xyz):
    """alias: the LAST atom with the same coordinate."""
    last = {}
    for i, p in enumerate(xyz):
        last[p.tobytes()] = i
    return np.array([last[p.tobytes()] for p in xyz], dtype=np.int32)


def chain_entry(xyz, radius, weight, residue, cutoff, min_electrons=25.0):
    """A key per atom, bonds to the neighbours i - 2, i - 1, i + 1, i + 2 inside the residue, every atom an owner."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    residue = np.asarray(residue, dtype=np.int32)
    cand = np.arange(n)[:, None] + np.array([-2, -1, 1, 2])[None, :]
    valid = (cand >= 0) & (cand < n)
    valid &= residue[np.clip(cand, 0, max(n - 1, 0))] == residue[:, None] if n else valid
    return {"xyz": xyz, "radius": np.asarray(radius, dtype=np.float32), "weight": np.asarray(weight, dtype=np.float64), "residue": residue,
            "alias": last_of_coordinate(xyz), "key": np.arange(n, dtype=np.int32),
            "bonded_off": np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int64), "bonded": cand[valid].astype(np.int32),
            "owner_key": np.arange(n, dtype=np.int32), "cutoff": float(np.float32(cutoff)), "min_electrons": float(min_electrons)}


def prefix(e, n):
    """The first n atoms of a chain_entry() as an entry of its own (a residue cut by the prefix is a shorter residue)."""
    return chain_entry(e["xyz"][:n], e["radius"][:n], e["weight"][:n], e["residue"][:n], e["cutoff"], e["min_electrons"])


# ---- 1. the large entry -----------------------------------------------------------------------------------------------------
BIG_NCRS = 224
BIG_SITES = 48000
SPLIT_SHARE = 0.12
JITTER = 0.3
BIG_SIZES = (11000, 19000, 29000, 48000)          # below T2 < T1 < T3, between each neighbouring pair, above all (tests/test_cloud_host.py states the three and asserts the sides)
_big = {}


def big_entry():
    """(spec, header, grid, entry).  Sites on strips of triangles of side 1.55 A along x (atoms i - 2 .. i + 2 are neighbours), 2.5 A between the strips,
    jittered by +-JITTER, float32 promoted to double; residues of 6-10 consecutive atoms; a Gaussian (sigma 0.6 A) at every site, tall
    enough to fill most of the atom's sphere -- 2 % of them too faint for the cut-off, so that such an atom has no cloud of its own and
    catches the edges of its neighbours' -- and white noise.  At SPLIT_SHARE of the sites the plane of voxels through the site's voxel
    (across a random axis; across two axes at a tenth of them) is zeroed: what is left of the sphere on either side are two (four) clouds."""
    if "e" in _big:
        return _big["e"]
    from pdb_eda_amd import synthetic
    rng = np.random.default_rng(20240611)
    n, N, h = BIG_SITES, BIG_NCRS, 0.5
    spec = synthetic.MapSpec(ncrs=(N, N, N), spacing=h)
    header = header_of(spec)
    px, rung, pyz = 1.55, 1.35, 2.5          # a strip of near-equilateral triangles along x: atoms i - 2 .. i + 2 are all neighbours of atom i
    nx, ny = 2 * int((N * h - 5.0) / px), int((N * h - 5.0) / (rung + pyz))
    i = np.arange(n)
    lattice = np.stack([2.0 + 0.5 * px * (i % nx), 2.0 + (rung + pyz) * ((i // nx) % ny) + rung * (i % 2), 2.0 + pyz * (i // (nx * ny))], axis=1)
    assert lattice.max() < N * h - 2.0
    xyz = (lattice + rng.uniform(-JITTER, JITTER, size=(n, 3))).astype(np.float32).astype(np.float64)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(6, 11)))
    residue = np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int32)
    radius = rng.choice(np.array([0.74, 0.8, 0.9], dtype=np.float32), size=n)
    weight = np.round(rng.uniform(5.0, 9.0, size=n), 3) + 1e-6 * (i % 1000)          # (electrons that identify the members of a row)
    amp = np.where(rng.random(n) < 0.02, 0.2, rng.uniform(1.4, 2.4, size=n))
    # the Gaussians: every site adds to the 7^3 voxels around its nearest voxel, one bincount per 8 000 sites
    off = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    centre = np.rint(xyz / h).astype(np.int64)
    grid = np.zeros(N ** 3, dtype=np.float64)
    for a in range(0, n, 8000):
        vox = centre[a:a + 8000, None, :] + off[None, :, :]
        d2 = ((vox * h - xyz[a:a + 8000, None, :]) ** 2).sum(axis=2)
        val = amp[a:a + 8000, None] * np.exp(-d2 / (2 * 0.6 ** 2))
        flat = (vox[:, :, 2] * N + vox[:, :, 1]) * N + vox[:, :, 0]          # [s][r][c], c fastest; x -> c, y -> r, z -> s
        grid += np.bincount(flat.reshape(-1), weights=val.reshape(-1), minlength=N ** 3)
    grid += 0.05 * rng.standard_normal(N ** 3, dtype=np.float32)
    split = np.nonzero(rng.random(n) < SPLIT_SHARE)[0]
    plane = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), indexing="ij"), axis=-1).reshape(-1, 2)
    for who in (split, split[rng.random(len(split)) < 0.1]):
        axis = rng.integers(0, 3, size=len(who))
        for ax in range(3):
            mine = who[axis == ax]
            o = np.zeros((len(plane), 3), dtype=np.int64)
            o[:, [k for k in range(3) if k != ax]] = plane
            at = centre[mine, None, :] + o[None, :, :]
            grid[((at[:, :, 2] * N + at[:, :, 1]) * N + at[:, :, 0]).reshape(-1)] = 0.0
    grid = np.ascontiguousarray(grid.reshape(N, N, N), dtype=np.float32)
    _big["e"] = (spec, header, grid, chain_entry(xyz, radius, weight, residue, 0.5))
    return _big["e"]


# ---- 2. atoms that leave the stored box, and many clouds an atom -------------------------------------------------------------
WORLD_ATOMS = 400


def world_entry(name, kind):
    """(spec, header, grid, entry) of world ``name`` ("orth": everything wraps; "skew": triclinic, permuted axes, crsStart != 0, part
    of the cell not stored).  kind "smooth": the world's own map, radii 0.74-0.9, the cut-off at mean + 0.25 std (about half of the atoms have a cloud);  kind "noise": unit
    white noise, radius 3.0, the cut-off at mean + 1 std."""
    spec, grid = batch_limit_cases.spec_and_grid(name)
    header = header_of(spec)
    xyz = batch_limit_cases.base_atoms(name, header)[:WORLD_ATOMS]
    rng = np.random.default_rng(311 + batch_limit_cases.WORLDS.index(name))
    n = len(xyz)
    if kind == "noise":
        grid = np.random.default_rng(5200 + batch_limit_cases.WORLDS.index(name)).standard_normal(grid.shape, dtype=np.float32)
        radius, sigmas = np.full(n, 3.0, dtype=np.float32), 1.0
    else:
        radius, sigmas = rng.choice(np.array([0.74, 0.8, 0.9], dtype=np.float32), size=n), 0.25
    g = grid.astype(np.float64)
    weight = np.round(rng.uniform(5.0, 9.0, size=n), 3) + 1e-6 * np.arange(n)
    return spec, header, grid, chain_entry(xyz, radius, weight, np.arange(n) // 8, g.mean() + sigmas * g.std(), min_electrons=12.0)


# ---- 3. crafted decision cases -------------------------------------------------------------------------------------------------
CRAFT_NCRS = 40
CRAFT_CUTOFF = 0.5          # every painted voxel is >= 1, everything else is 0


class _Case(object):
    """Atoms on voxel centres around ``origin`` and the voxels painted for them."""

    def __init__(self, grid, origin, min_electrons=25.0):
        self.grid, self.origin, self.min_electrons = grid, np.array(origin), min_electrons
        self.atoms, self.bonds, self.owners, self.alias = [], {}, None, {}

    def paint(self, crs, value):
        c, r, s = (self.origin + crs) % CRAFT_NCRS
        assert self.grid[s, r, c] == 0.0 and value * 64 == int(value * 64) and 1.0 <= value <= 8.0
        self.grid[s, r, c] = value

    def atom(self, crs, radius, weight, residue, key=None, paint=None):
        """An atom on the centre of voxel ``crs``; paint: the density of that voxel.  Returns the atom's index."""
        if paint is not None:
            self.paint(crs, paint)
        self.atoms.append((tuple(int(x) for x in self.origin + crs), radius, weight, residue, len(self.atoms) if key is None else key))
        return len(self.atoms) - 1

    def bond(self, k1, k2):
        self.bonds.setdefault(k1, []).append(k2)
        self.bonds.setdefault(k2, []).append(k1)

    def entry(self, header):
        n = len(self.atoms)
        xyz = np.array([header.crs2xyzCoord(list(a[0])) for a in self.atoms], dtype=np.float64).reshape(n, 3)
        key = np.array([a[4] for a in self.atoms], dtype=np.int32)
        n_keys = int(key.max()) + 1 if n else 0
        per_key = [self.bonds.get(k, []) for k in range(n_keys)]
        alias = last_of_coordinate(xyz)
        for i, j in self.alias.items():
            alias[i] = j
        owners = key if self.owners is None else self.owners
        return {"xyz": xyz, "radius": np.array([a[1] for a in self.atoms], dtype=np.float32), "weight": np.array([a[2] for a in self.atoms], dtype=np.float64),
                "residue": np.array([a[3] for a in self.atoms], dtype=np.int32), "alias": alias, "key": key,
                "bonded_off": np.concatenate([[0], np.cumsum([len(b) for b in per_key])]).astype(np.int64),
                "bonded": np.array([k for b in per_key for k in b], dtype=np.int32), "owner_key": np.asarray(owners, dtype=np.int32),
                "cutoff": CRAFT_CUTOFF, "min_electrons": float(self.min_electrons)}


SELF = 0.3          # a sphere that holds the atom's own voxel alone (0.6 voxels)
_crafted = {}


def crafted():
    """(spec, header, grid, {case: entry}).  Every case lives in a region of its own, 12 voxels from the next along y and z: no
    sphere of one case reaches a voxel painted for another, and no painted voxels of two cases touch."""
    if "c" in _crafted:
        return _crafted["c"]
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(CRAFT_NCRS,) * 3, spacing=0.5)
    header = header_of(spec)
    grid = np.zeros((CRAFT_NCRS,) * 3, dtype=np.float32)
    cases = {}

    # equidistant: two clouds mirrored about the atom (2 voxels = 1.0 A either side), 2.0 and 3.0: the row carries the first in list order
    c = _Case(grid, (6, 6, 6))
    c.atom((0, 0, 0), 1.25, 7.0, 0)
    c.paint((-2, 0, 0), 2.0); c.paint((2, 0, 0), 3.0)
    c.atom((8, 0, 0), SELF, 30.0, 0, paint=1.0)
    cases["equidistant"] = c

    # cut-off: six atoms on their own voxel (distance 0) and two atoms with two clouds each, the nearest 2 voxels (X) and 3 voxels (Y)
    # away: median 0, std 0.5555 A, cut-off 1.3887 A = 2.777 voxels -- X is 0.777 voxels inside, Y 0.223 voxels outside
    c = _Case(grid, (4, 18, 6), min_electrons=0.0)
    for k in range(6):
        c.atom((3 * k, 0, 0), SELF, 6.0 + k, 0, paint=1.0 + k / 64.0)
    c.atom((21, 0, 0), 1.6, 7.5, 1); c.paint((19, 0, 0), 2.0); c.paint((21, 2, 2), 2.5)
    c.atom((29, 0, 0), 1.6, 8.5, 1); c.paint((26, 0, 0), 3.0); c.paint((29, 3, 1), 3.5)
    cases["cutoff"] = c

    # electron threshold: a residue of 8 + 8 + 9 = 25.0 electrons in one cloud (kept by >=), a residue of 8 + 8 + (9 - 2^-40) (filtered)
    c = _Case(grid, (6, 30, 6))
    for r, last in ((0, 9.0), (1, 9.0 - 2.0 ** -40)):
        for k, w in enumerate((8.0, 8.0, last)):
            c.atom((10 * r + k, 0, 0), SELF, w, r, paint=1.0 + (3 * r + k) / 8.0)
    cases["threshold"] = c

    # corner contact: a bonded pair at offset (1, 1, 1) and a twin at (2, 2, 2)
    c = _Case(grid, (6, 6, 18), min_electrons=0.0)
    for r, step in ((0, 1), (1, 2)):
        a = c.atom((10 * r, 0, 0), SELF, 6.0 + r, r, paint=1.5 + r)
        b = c.atom((10 * r + step, step, step), SELF, 7.5 + r, r, paint=2.25 + r)
        c.bond(a, b)
    cases["corner"] = c

    # chained residue: A touches B (edge), B touches C (edge), A and C are 3 voxels apart
    c = _Case(grid, (6, 18, 18))
    a = c.atom((0, 0, 0), SELF, 9.0, 0, paint=1.0)
    b = c.atom((1, 1, 0), 0.6, 10.0, 0, paint=2.0); c.paint((2, 1, 0), 1.25)
    d = c.atom((3, 0, 0), SELF, 11.0, 0, paint=4.0)
    c.bond(a, b); c.bond(b, d); c.bond(a, d)
    cases["chain"] = c

    # residue ordinals 3, 3, 3, 5, 7, 7, 12: residue 5 has no cloud; in residue 3 a key comes twice -- its first atom's cloud touches the
    # bonded partner's, its last atom's does not (the last atom of a name wins: the owners of that key are incomplete)
    c = _Case(grid, (4, 30, 18), min_electrons=0.0)
    a = c.atom((0, 0, 0), SELF, 6.0, 3, key=0, paint=1.0)
    b = c.atom((1, 0, 0), SELF, 7.0, 3, key=1, paint=1.5)
    c.atom((4, 0, 0), SELF, 8.0, 3, key=0, paint=2.0)
    c.atom((8, 0, 0), SELF, 6.5, 5, key=2)
    c.atom((12, 0, 0), SELF, 7.0, 7, key=3, paint=2.5); c.atom((13, 0, 0), SELF, 7.5, 7, key=4, paint=3.0)
    c.atom((17, 0, 0), SELF, 8.0, 12, key=5, paint=3.5)
    c.bond(0, 1); c.bond(3, 4)
    cases["ordinals"] = c

    # aliases: (i) two atoms of residue 0 on one coordinate: the residue cloud has the later atom's electrons only; (ii) an atom of
    # residue 1 and one of residue 2 on one coordinate: both count; (iii) an atom of residue 3 (radius: its own voxel) on the coordinate
    # of a later atom of residue 4 with a 0.6 A sphere: the earlier atom's row carries the larger cloud
    c = _Case(grid, (4, 6, 30), min_electrons=0.0)
    c.atom((0, 0, 0), SELF, 6.0, 0, paint=1.0); c.atom((0, 0, 0), SELF, 7.0, 0); c.atom((1, 0, 0), SELF, 8.0, 0, paint=1.5)
    c.atom((8, 0, 0), SELF, 6.5, 1, paint=2.0); c.atom((8, 0, 0), SELF, 7.5, 2)
    c.atom((16, 0, 0), SELF, 5.5, 3, paint=2.5); c.atom((16, 0, 0), 0.6, 8.5, 4); c.paint((17, 0, 0), 3.0)
    cases["aliases"] = c

    # no bonded entries and no owners, on pooled clouds
    c = _Case(grid, (6, 18, 30))
    c.atom((0, 0, 0), SELF, 30.0, 0, paint=1.0); c.atom((1, 0, 0), SELF, 31.0, 0, paint=2.0); c.atom((6, 0, 0), SELF, 32.0, 1, paint=3.0)
    c.owners = np.zeros(0, dtype=np.int32)
    cases["no_pairs"] = c

    entries = {k: v.entry(header) for k, v in cases.items()}
    assert grid.max() <= 8.0 and np.all(grid * 64 == np.rint(grid * 64))
    # no pooled cloud: the cut-off above the map's maximum
    entries["nothing"] = dict(entries["chain"], cutoff=9.0)
    entries["empty"] = chain_entry(np.zeros((0, 3)), [], [], [], CRAFT_CUTOFF)
    _crafted["c"] = (spec, header, grid, entries)
    return _crafted["c"]


def refusals(e):
    """{what: entry}: entry e with one argument that pdbeda_aggregate_cloud refuses (PDBEDA_ERR_ARGUMENT)."""
    def changed(field, index, value):
        a = e[field].copy()
        a[index] = value
        return dict(e, **{field: a})
    n, n_keys = len(e["xyz"]), len(e["bonded_off"]) - 1
    assert n >= 3 and len(e["bonded"]) and len(e["owner_key"])
    return {"alias out of range": changed("alias", 1, n), "key out of range": changed("key", 1, n_keys),
            "decreasing residues": changed("residue", n - 1, int(e["residue"][0]) - 1), "owner key out of range": changed("owner_key", 0, n_keys),
            "bonded key out of range": changed("bonded", 0, n_keys)}


def device_map(spec, grid, name, ctx):
    from pdb_eda_amd import ccp4, synthetic
    return ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), name, ctx=ctx)
