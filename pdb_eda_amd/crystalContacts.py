"""pdb_eda ``contacts`` mode (reference crystalContacts.py) on the GPU, without pymol.

The reference asks pymol's ``symexp`` for the symmetry mates of the entry's ``polymer`` selection that come within the cutoff
of it and then takes, for every query atom, the minimum ``scipy.spatial.distance.cdist`` distance to their atoms.  Here the
same set follows from what the analysis already has: the asymmetric unit's atoms, the REMARK 290 operators and the cell.

* P = the polymer atoms: those of residues whose hetero flag is blank (ATOM records), one per atom name as ``read_pdb`` keeps them.
* An image g = (op k, n in Z^3) maps x to R_k x + t_k + orthoMat n, with the arithmetic of the symmetry atoms (for |n| <= 1 an
  image coordinate equals the matching ``symmetryAtomCoords`` entry bit for bit).  (op 0, n = 0) is the asymmetric unit, never an image.
* g is kept iff min over i, j in P of |x_i - g(x_j)| <= cutoff; the neighbour set N is the union of g(P) over the kept g.
* The contact of a query q is min over y in N of |q - y| (fp64, sqrt((dx*dx + dy*dy) + dz*dz) as cdist), reported when <= cutoff.

Differences from the reference (pymol): pymol stores coordinates as float32 (distances differ in about the 7th digit); its
``polymer`` selection counts modified residues written as HETATM (MSE, ...), which count as ligands here; it loads every altloc;
it searches a fixed range of cell shifts, while :func:`candidateImages` enumerates every image that can come within the cutoff;
and where no image is kept the reference fails in ``np.min`` of an empty array, while here the result has no rows.

There is no docopt command line (as in :mod:`singleStructure`): :func:`rows` returns the table and ``singleStructure.write`` /
``dumps`` write it as the reference does.
"""
import numpy as np

from . import _native
from . import structure as _structure

headerList = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", "symmetry", "xyz", "crystal_contact_distance"]


def _ctx(ctx):
    return ctx if ctx is not None else _native.default_context()


def findCoordContacts(coordList1, coordList2, distanceCutoff=5.0, ctx=None):
    """Contacts of coordList1 to coordList2 at the given distance cutoff (ref crystalContacts.py:87-101): a list of
    ``(index, minDistance)`` for the points of coordList1 whose nearest coordList2 point is within the cutoff (boundary
    included), in ascending index.  A cell-list search on the device instead of a dense cdist matrix."""
    idx, dist = _ctx(ctx).coord_contacts(np.asarray(coordList1, dtype=np.float64).reshape(-1, 3),
                                         np.asarray(coordList2, dtype=np.float64).reshape(-1, 3), float(distanceCutoff))
    return list(zip(idx.tolist(), dist.tolist()))


def _rotations(rotationMats):
    return np.array([np.asarray(m, dtype=np.float64).reshape(3, 4) for m in rotationMats], dtype=np.float64).reshape(-1, 3, 4)


def candidateImages(rotationMats, orthoMat, polyCoords, cutoff):
    """Every image (op, n0, n1, n2) that can bring a polymer atom within ``cutoff`` of another, as an int32 (m, 4) array in
    (op, n) order; (op 0, n = 0) is left out.  Complete: an image g is kept iff some x_i - R x_j - t = orthoMat n + e with
    |e| <= cutoff, so orthoMat n lies in the box of x_i - R x_j - t over P grown by the cutoff, and n in the box of that box's
    8 corners mapped through the inverse cell.  The device decides which of these are kept."""
    rot = _rotations(rotationMats)
    p = np.asarray(polyCoords, dtype=np.float64).reshape(-1, 3)
    if len(p) == 0 or len(rot) == 0:
        return np.zeros((0, 4), dtype=np.int32)
    deortho = np.linalg.inv(np.asarray(orthoMat, dtype=np.float64).reshape(3, 3))
    plo, phi = p.min(axis=0), p.max(axis=0)
    grow = float(cutoff) * (1.0 + 1e-6) + 1e-6 * (1.0 + float(np.abs(p).max()))     # (rounding: a candidate too many costs nothing)
    out = []
    for k, m in enumerate(rot):
        moved = p.dot(m[:, :3].T) + m[:, 3]
        lo = plo - moved.max(axis=0) - grow
        hi = phi - moved.min(axis=0) + grow
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        frac = corners.dot(deortho.T)
        nlo = np.floor(frac.min(axis=0)).astype(np.int64)
        nhi = np.ceil(frac.max(axis=0)).astype(np.int64)
        grid = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(nlo, nhi)], indexing="ij"), axis=-1).reshape(-1, 3)
        if k == 0:
            grid = grid[np.any(grid != 0, axis=1)]
        out.append(np.hstack([np.full((len(grid), 1), k, dtype=np.int64), grid]))
    return np.concatenate(out).astype(np.int32)


def polymerCoordinates(analyzer):
    """P: the coordinates (float64) of the atoms of residues whose hetero flag is blank."""
    cols = _structure.columns(analyzer.biopdbObj)
    het = np.asarray(cols.res_het, dtype=bool)[np.asarray(cols.res_of_atom, dtype=np.int64)] if len(cols.coord) else np.zeros(0, dtype=bool)
    return np.ascontiguousarray(cols.coord[~het], dtype=np.float64)


def _cell(analyzer):
    rot = _rotations(analyzer.pdbObj.header.rotationMats)
    ortho = np.asarray(analyzer.densityObj.header.orthoMat, dtype=np.float64).reshape(3, 3)
    return rot, ortho


def keptImages(analyzer, distanceCutoff=5.0):
    """The kept images (int32 (m, 4) array of (op, n0, n1, n2)) and P."""
    poly = polymerCoordinates(analyzer)
    rot, ortho = _cell(analyzer)
    cand = candidateImages(rot, ortho, poly, distanceCutoff)
    kept, _, _ = analyzer.densityObj._ctx.crystal_contacts(np.zeros((0, 3)), poly, rot, ortho, cand, float(distanceCutoff))
    return cand[kept], poly


def simulateCrystalNeighborCoordinates(analyzer, distanceCutoff=5.0):
    """N: the atoms of the kept images in (op, n, atom) order, an (m, 3) float64 array (ref crystalContacts.py:104-142,
    there a list from pymol)."""
    images, poly = keptImages(analyzer, distanceCutoff)
    rot, ortho = _cell(analyzer)
    return analyzer.densityObj._ctx.image_coords(poly, rot, ortho, images)


def contacts(analyzer, distance=5.0, symmetryAtoms=False):
    """(query atoms, [(index, minDistance)]) of ``main`` (crystalContacts.py:58-66): the kept images and the contacts in one device call."""
    if symmetryAtoms:
        atoms = analyzer.symmetryAtoms
        query = np.asarray(analyzer.symmetryAtomCoords, dtype=np.float64).reshape(-1, 3)
    else:
        atoms = list(analyzer.biopdbObj.get_atoms())
        query = _structure.columns(analyzer.biopdbObj).coord
    poly = polymerCoordinates(analyzer)
    rot, ortho = _cell(analyzer)
    cand = candidateImages(rot, ortho, poly, distance)
    _, idx, dist = analyzer.densityObj._ctx.crystal_contacts(query, poly, rot, ortho, cand, float(distance))
    return atoms, list(zip(idx.tolist(), dist.tolist()))


def rows(analyzer, distance=5.0, symmetryAtoms=False, includePdbid=False):
    """``(headerList, result)`` exactly as ``main`` builds them (crystalContacts.py:58-77); write them with
    ``singleStructure.write`` / ``dumps``."""
    atoms, found = contacts(analyzer, distance, symmetryAtoms)
    header = list(headerList)
    result = []
    for index, contactDistance in found:
        atom = atoms[index]
        result.append([atom.parent.parent.parent.id, atom.parent.parent.id, atom.parent.id[1], atom.parent.resname, atom.name, atom.get_occupancy(),
                       [x for x in atom.symmetry] if symmetryAtoms else [0, 0, 0, 0], [float(c) for c in atom.coord], contactDistance])
    if includePdbid:
        header = ["pdbid"] + header
        result = [[analyzer.pdbid] + row for row in result]
    return header, result
