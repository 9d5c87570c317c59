"""Electron-density analysis on MI355X behind pdb_eda's ``densityAnalysis`` API surface.

Mirrors ``pdb_eda/densityAnalysis.py`` (``fromFile``/``fromPDBid``/``DensityAnalysis`` with the
reference's attribute, method and result-header names) for the rows of the accelerated path:
blob lists, ``aggregateCloud``, ``calculateAtomSpecificBlobStatistics``, region density /
discrepancy.  All voxel work -- sphere gathers, clustering, unions, regional sums, symmetry
atoms, nearest atom -- runs in ``libpdbeda_hip.so``; what stays on the host is the reference's
own host-side tail: per-atom table bookkeeping and the numpy/scipy statistics over <= nAtoms rows
(densityAnalysis.py:734-767).  Out of scope: downloads, RSCC/RSR, F000.

Parameters (radii, slopes, electrons, bonded atoms) are *reference data*: they are not shipped.
Load the reference's ``conf/optimized_params.json`` (or your own) with :func:`loadParams` /
:func:`setGlobals`, or set ``PDB_EDA_PARAMS``.
"""
import collections
import gzip
import json
import math
import operator
import os

import numpy as np

from . import ccp4
from . import structure as _structure

paramsGlobal = None
radiiGlobal = None
slopesGlobal = None
bondedAtomsGlobal = None
fullAtomNameMapElectronsGlobal = None
fullAtomNameMapAtomTypeGlobal = None
atomTypeLengthGlobal = None

ccp4folder = './ccp4_data/'
pdbfolder = './pdb_data/'

# the calculated (model) density: added to every B-factor (A^2), and the cut-off of an atom in standard deviations of its Gaussian
modelBlur = 0.0
modelSigmas = ccp4.MODEL_N_SIGMA
refineCycles = 5          # cycles of ``refineAtoms`` / the "refine" mode
refineMaxShift = 0.3      # A: the longest shift of an atom in one refinement cycle
fitRotations = 4096       # rotations of the lattice pass of ``fitFragment`` / the "fit" mode
fitPenaltyCutoffs = 3.0   # the clash penalty of ``fitFragment``, in units of the Fo-Fc map's ``diffDensityCutoff``
fitMinVolumePerAtom = 0.5   # A^3 of blob per fragment atom below which ``calculateBlobFits`` skips a blob
fitMaxCentres = 2000      # the most voxel centres of a blob that ``fitFragment`` tries (a larger blob is thinned evenly)

# the local statistics of a map: the Gaussian window's standard deviation (A) and cut-off (standard deviations), and the floor under a local
# standard deviation as a fraction of the whole map's stdDensity (a flat solvent region must not turn rounding noise into z-scores)
localWindowSigma = 3.0
localWindowTruncate = 3.0
localStdFloorFraction = 0.25


def setGlobals(params):
    """ref densityAnalysis.py:48-68."""
    global paramsGlobal, radiiGlobal, slopesGlobal, bondedAtomsGlobal
    global fullAtomNameMapElectronsGlobal, fullAtomNameMapAtomTypeGlobal, atomTypeLengthGlobal
    paramsGlobal = params
    radiiGlobal = params['radii']
    slopesGlobal = params['slopes']
    bondedAtomsGlobal = params['bonded_atoms']
    fullAtomNameMapElectronsGlobal = params['full_atom_name_map_electrons']
    fullAtomNameMapAtomTypeGlobal = params['full_atom_name_map_atom_type']
    atomTypeLengthGlobal = max(len(t) for t in fullAtomNameMapAtomTypeGlobal.values()) + 5


def loadParams(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, 'rt') as fh:
        setGlobals(json.load(fh))


if os.environ.get("PDB_EDA_PARAMS"):
    loadParams(os.environ["PDB_EDA_PARAMS"])


def _requireParams():
    if paramsGlobal is None:
        raise RuntimeError("no analysis parameters loaded: call pdb_eda_amd.densityAnalysis.loadParams(<optimized_params.json>) "
                           "or set PDB_EDA_PARAMS (the reference's parameter tables are data and are not shipped)")


def fromFile(pdbFile, ccp4DensityFile=None, ccp4DiffDensityFile=None, ctx=None):
    """ref densityAnalysis.py:182-229; returns 0 on any failure, like the reference."""
    pdbid = "xxxx"
    densityObj = None
    diffDensityObj = None
    try:
        if ccp4DensityFile is not None:
            densityObj = ccp4.read(ccp4DensityFile, pdbid, ctx=ctx) if isinstance(ccp4DensityFile, str) else ccp4.parse(ccp4DensityFile, pdbid, ctx=ctx)
            _attachCutoffs(densityObj, None)
        if ccp4DiffDensityFile is not None:
            diffDensityObj = ccp4.read(ccp4DiffDensityFile, pdbid, ctx=ctx) if isinstance(ccp4DiffDensityFile, str) else ccp4.parse(ccp4DiffDensityFile, pdbid, ctx=ctx)
            _attachCutoffs(None, diffDensityObj)
        biopdbObj, pdbObj = _structure.read_pdb(pdbFile, pdbid)
    except Exception:
        return 0
    return DensityAnalysis(pdbid, densityObj, diffDensityObj, biopdbObj, pdbObj)


def fromPDBid(pdbid, ccp4density=True, ccp4diff=True, pdbbio=True, pdbi=True, downloadFile=True, mmcif=False):
    """ref densityAnalysis.py:88-179 for files already present under ./ccp4_data and ./pdb_data
    (there is no network here: nothing is downloaded; a missing file gives 0 like a failed download)."""
    pdbid = pdbid.lower()
    try:
        densityObj = diffDensityObj = biopdbObj = pdbObj = None
        if ccp4density:
            densityObj = ccp4.read(ccp4folder + pdbid + '.ccp4', pdbid)
            _attachCutoffs(densityObj, None)
        if ccp4diff:
            diffDensityObj = ccp4.read(ccp4folder + pdbid + '_diff.ccp4', pdbid)
            _attachCutoffs(None, diffDensityObj)
        if pdbbio or pdbi:
            biopdbObj, pdbObj = _structure.read_pdb(pdbfolder + 'pdb' + pdbid + '.ent.gz', pdbid)
    except Exception:
        return 0
    return DensityAnalysis(pdbid, densityObj, diffDensityObj, biopdbObj, pdbObj)


def _attachCutoffs(densityObj, diffDensityObj):
    """ref densityAnalysis.py:131-132, 148."""
    if densityObj is not None:
        densityObj.densityCutoff = densityObj.meanDensity + 1.5 * densityObj.stdDensity
        densityObj.densityCutoffFromHeader = densityObj.header.densityMean + 1.5 * densityObj.header.rmsd
    if diffDensityObj is not None and getattr(diffDensityObj, "resident", True):
        diffDensityObj.diffDensityCutoff = diffDensityObj.meanDensity + 3 * diffDensityObj.stdDensity
    # (a lazily read Fo-Fc map computes the same value when it is first asked for: ccp4.DensityMatrix.diffDensityCutoff)


def residueAtomName(atom):
    """ref densityAnalysis.py:1243-1252."""
    return atom.parent.resname.strip() + '_' + atom.name


def fragmentFromResidue(residue):
    """A rigid fragment from the object model: a dict ``xyz`` (n, 3) float64, ``electrons`` (n,: the parameter tables' electrons of
    'RES_ATOM' times the occupancy; an atom the tables do not know counts by its element's atomic number, 6 when that is unknown too),
    ``elements`` and ``names`` -- what ``DensityAnalysis.fitFragment`` takes.  Atoms of occupancy 0 are left out."""
    _requireParams()
    numbers = {"H": 1.0, "C": 6.0, "N": 7.0, "O": 8.0, "F": 9.0, "NA": 11.0, "MG": 12.0, "P": 15.0, "S": 16.0, "CL": 17.0, "K": 19.0, "CA": 20.0, "FE": 26.0, "ZN": 30.0}
    xyz, electrons, elements, names = [], [], [], []
    for atom in residue.child_list:
        if float(atom.occupancy) == 0.0:
            continue
        name = residueAtomName(atom)
        z = fullAtomNameMapElectronsGlobal.get(name) if fullAtomNameMapElectronsGlobal else None
        element = (getattr(atom, "element", "") or "").strip().upper()
        xyz.append(np.asarray(atom.coord, dtype=np.float64))
        electrons.append((float(z) if z is not None else numbers.get(element, 6.0)) * float(atom.occupancy))
        elements.append(element)
        names.append(atom.name)
    return {"xyz": np.array(xyz, dtype=np.float64).reshape(-1, 3), "electrons": np.array(electrons, dtype=np.float64), "elements": elements, "names": names}


class SymAtom(object):
    """ref cutils.pyx:105-123: an atom with its own symmetry tag and coordinate."""

    def __init__(self, atom, coord, symmetry):
        self.atom = atom
        self.coord = coord
        self.symmetry = symmetry

    def __getattr__(self, attr):
        return getattr(self.atom, attr)


def _typeRegressions(x, y, bfactor, group, n_types):
    """``scipy.stats.linregress(x[sel], y[sel])`` for every atom type at once (ref densityAnalysis.py:752-757 calls it per type:
    five calls were 0.3 ms of a 500-atom entry's 3 ms).  Returns (slope, two-sided p-value, fitted) per type, where ``fitted`` is
    the reference's own condition for fitting at all: more than two rows and not all b-factors equal.  Same formulas as scipy
    (biased covariances about the means, r clipped to [-1, 1], t = r sqrt(df / ((1 - r + TINY)(1 + r + TINY))), p = 2 stdtr(df, -|t|)),
    with the sums taken per type by ``np.bincount``; pinned against scipy itself in tests/test_structure.py."""
    from scipy import special
    n = np.bincount(group, minlength=n_types).astype(np.float64)
    safe_n = np.maximum(n, 1.0)
    xm = np.bincount(group, weights=x, minlength=n_types) / safe_n
    ym = np.bincount(group, weights=y, minlength=n_types) / safe_n
    dx, dy = x - xm[group], y - ym[group]
    ssxm = np.bincount(group, weights=dx * dx, minlength=n_types) / safe_n
    ssym = np.bincount(group, weights=dy * dy, minlength=n_types) / safe_n
    ssxym = np.bincount(group, weights=dx * dy, minlength=n_types) / safe_n
    order = np.argsort(group, kind="stable")
    first = np.searchsorted(group[order], np.arange(n_types))
    present = n > 0
    b_sorted = bfactor[order]
    # the reference's test is `len(np.unique(bfactor)) == 1` (densityAnalysis.py:752), and np.unique counts all NaNs as ONE value:
    # a type whose b-factors are all NaN (no positive B: its median is NaN, and so is every normalised value) is NOT fitted
    b_lo = np.where(present, np.fmin.reduceat(b_sorted, np.minimum(first, max(len(b_sorted) - 1, 0))), 0.0) if len(b_sorted) else np.zeros(n_types)
    b_hi = np.where(present, np.fmax.reduceat(b_sorted, np.minimum(first, max(len(b_sorted) - 1, 0))), 0.0) if len(b_sorted) else np.zeros(n_types)
    n_nan = np.bincount(group, weights=np.isnan(bfactor), minlength=n_types)
    one_value = (n_nan == n) | ((n_nan == 0) & (b_lo == b_hi))
    fitted = (n > 2) & ~one_value
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((ssxm == 0.0) | (ssym == 0.0), 0.0, ssxym / np.sqrt(ssxm * ssym))
        r = np.clip(r, -1.0, 1.0)
        slope = ssxym / ssxm
        df = n - 2.0
        t = r * np.sqrt(df / ((1.0 - r + 1.0e-20) * (1.0 + r + 1.0e-20)))
        p = 2.0 * special.stdtr(np.maximum(df, 1.0), -np.abs(t))
    return slope, p, fitted


def _lastWithSameCoord(coord32):
    """For every row of float32 coordinates, the index of the LAST row with an equal triple (``allAtomClouds[tuple(atom.coord)]``
    keeps the last atom of a coordinate, ref densityAnalysis.py:604; equal as floats: -0.0 is 0.0).  One 64-bit sort of a mixed
    key instead of a sort of 12-byte records; rows whose keys collide without being equal send the call to the slow exact path."""
    n = len(coord32)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    bits = np.ascontiguousarray(coord32 + np.float32(0.0)).view(np.uint32).astype(np.uint64)     # (+0.0: -0.0 becomes 0.0)
    key = ((bits[:, 0] << np.uint64(32)) | bits[:, 1]) * np.uint64(0x9E3779B97F4A7C15) ^ (bits[:, 2] * np.uint64(0xC2B2AE3D27D4EB4F))
    order = np.argsort(key, kind="stable")
    sorted_bits, sorted_key = bits[order], key[order]
    same_row = (sorted_bits[1:] == sorted_bits[:-1]).all(axis=1)
    if ((sorted_key[1:] == sorted_key[:-1]) & ~same_row).any():
        triple = np.ascontiguousarray(bits.astype(np.uint32)).view(np.dtype((np.void, 12))).ravel()
        _, same = np.unique(triple, return_inverse=True)
        last = np.full(int(same.max()) + 1, -1, dtype=np.int64)
        np.maximum.at(last, same.reshape(-1), np.arange(n))
        return last[same.reshape(-1)]
    starts = np.flatnonzero(np.concatenate([[True], ~same_row]))
    group = np.cumsum(np.concatenate([[0], (~same_row).astype(np.int64)]))
    alias = np.empty(n, dtype=np.int64)
    alias[order] = np.maximum.reduceat(order, starts)[group]
    return alias


_pairTableCache = collections.OrderedDict()


def _pairTables(names, n_pairs):
    """What the parameter tables say about a structure's distinct 'RES_ATOM' names (``structure.Columns.pair_names``): atom type,
    electrons, and the bonded names that exist among them (densityAnalysis.py:617-621, 653-656), as arrays over the names.
    Entries of one run share their names (the same residues with the same atoms, met in the same order) and the tables are the
    same objects from entry to entry, so the answer is kept per (names, tables): a few dict look-ups per entry instead of a
    Python loop over ~160 names and their bonded lists."""
    typeMap, electronsMap, bonded = fullAtomNameMapAtomTypeGlobal, fullAtomNameMapElectronsGlobal, bondedAtomsGlobal
    key = (tuple(names), id(typeMap), id(electronsMap), id(bonded))
    hit = _pairTableCache.get(key)
    if hit is not None and hit["tables"][0] is typeMap and hit["tables"][1] is electronsMap and hit["tables"][2] is bonded:
        _pairTableCache.move_to_end(key)
        return hit
    known = np.fromiter((name in typeMap for name in names), dtype=bool, count=len(names))
    pair_id = {name: k for k, name in enumerate(names)}
    pair_type = [typeMap[name] if name in typeMap else None for name in names] + [None] * (n_pairs - len(names))
    electrons = np.full(n_pairs, np.nan)
    nb_off = np.zeros(n_pairs + 1, dtype=np.int64)
    nb = []
    for k, name in enumerate(names):
        if name in electronsMap:
            electrons[k] = electronsMap[name]
        nb.extend(pair_id[other] for other in bonded.get(name, ()) if other in pair_id)
        nb_off[k + 1] = len(nb)
    nb_off[len(names) + 1:] = len(nb)
    type_names = sorted({t for t in pair_type if t is not None})
    type_id = {t: k for k, t in enumerate(type_names)}
    pair_type_id = np.asarray([type_id[t] if t is not None else -1 for t in pair_type], dtype=np.int64)
    hit = {"tables": (typeMap, electronsMap, bonded), "known": known, "pair_type": pair_type, "pair_type_id": pair_type_id, "type_names": type_names,
           "electrons": electrons, "nb_off": nb_off, "nb": np.asarray(nb, dtype=np.int64)}
    _pairTableCache[key] = hit
    while len(_pairTableCache) > 32:
        _pairTableCache.popitem(last=False)
    return hit


class _SymAtomList(object):
    """The list of SymAtom objects createSymmetryAtoms returns (cutils.pyx:73-103), materialised item by item; the tables that
    list thousands of them read whole columns instead (``columns``)."""

    def __init__(self, cols, idx, sym, xyz, ident, rows=None):
        self._cols, self._idx, self._sym, self._xyz, self._ident = cols, idx, sym, xyz, ident
        self._rows = np.arange(len(idx)) if rows is None else np.asarray(rows)
        self._made = {}

    def subset(self, rows):
        return _SymAtomList(self._cols, self._idx, self._sym, self._xyz, self._ident, self._rows[rows])

    def __len__(self):
        return len(self._rows)

    def columns(self, items=None, type=""):
        """(rows of the structure columns, symmetry operators as an n x 4 int64 array -- a tuple per row once ``_rows`` has made the table --,
        coordinates as the SymAtom objects would hold them) of the listed
        items (all by default), optionally only those whose atom name is ``type``."""
        r = self._rows if items is None else self._rows[np.asarray(items, dtype=np.int64)]
        atom_rows = self._idx[r]
        if type:
            keep = np.asarray(self._cols.name)[atom_rows] == type if len(r) else np.zeros(0, dtype=bool)
            r, atom_rows = r[keep], atom_rows[keep]
        symmetry = np.ascontiguousarray(self._sym[r], dtype=np.int64)      # (n x 4 ints: _rows makes the tuples)
        own = self._cols.atom_lists("coord")                               # (most listed atoms are the structure's own: their coordinate objects as they are)
        picked = atom_rows.tolist()
        coords = list(operator.itemgetter(*picked)(own)) if len(picked) > 1 else [own[a] for a in picked]
        moved = np.nonzero(~self._ident[r])[0]
        if len(moved):
            xyz = self._xyz[r[moved]]
            for k, row in zip(moved.tolist(), xyz):                          # (a row view per symmetry copy only: iterating every row was 0.2 ms of a 1 400-blob table)
                coords[k] = row
        return atom_rows, symmetry, coords

    def _make(self, r):
        atom = self._cols.atoms[int(self._idx[r])]
        return SymAtom(atom, atom.coord if self._ident[r] else self._xyz[r], tuple(int(v) for v in self._sym[r]))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        r = int(self._rows[i])
        if r not in self._made:
            self._made[r] = self._make(r)
        return self._made[r]

    def __iter__(self):
        return (self[k] for k in range(len(self)))


def _segmentMeans(values, counts):
    """``np.mean`` of consecutive segments of ``values`` (``counts`` items each), bit-equal to calling it per segment: rows of
    equal length are reduced together along their contiguous axis, which is the summation numpy uses for a 1-D array."""
    counts = np.asarray(counts, dtype=np.int64)
    start = np.cumsum(counts) - counts
    out = np.full(len(counts), np.nan)
    for k in np.unique(counts).tolist():
        if k == 0:
            continue
        which = np.nonzero(counts == k)[0]
        out[which] = np.add.reduce(values[start[which][:, None] + np.arange(k)[None, :]], axis=1) / k
    return out


def _partitionRollup(columns, offsets):
    """Per-residue sums of per-atom partition columns: ``columns`` are arrays over the picked atoms in residue order, residue k has the
    atoms offsets[k] .. offsets[k + 1] (none: zeros).  Integer columns stay integers."""
    offsets = np.asarray(offsets, dtype=np.int64)
    out = []
    for column in columns:
        column = np.asarray(column)
        running = np.concatenate([np.zeros(1, dtype=column.dtype), np.cumsum(column)]) if column.dtype.kind in "iu" else None
        if running is not None:
            out.append(running[offsets[1:]] - running[offsets[:-1]])
        else:      # (floats: each residue summed on its own, not a difference of running sums)
            out.append(np.array([math.fsum(column[a:b].tolist()) for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())], dtype=np.float64))
    return out


def _blobOwners(owner, crs, offsets):
    """Who owns the voxels of every blob: ``owner`` is the partition's int32 volume ([s][r][c] of the box, -1 = unowned), ``crs`` the blobs'
    voxels (n x 3, columns c, r, s) grouped by blob, blob k having rows offsets[k] .. offsets[k + 1].  Arrays over the blobs: num_voxels,
    unowned_voxels, num_owner_atoms, main_owner (the atom that owns most of the blob's voxels, ties to the lowest index; -1 when
    nobody owns any) and main_owner_voxels."""
    crs, offsets = np.asarray(crs, dtype=np.int64).reshape(-1, 3), np.asarray(offsets, dtype=np.int64)
    n_blobs = len(offsets) - 1
    sizes = np.diff(offsets)
    who = np.asarray(owner)[crs[:, 2], crs[:, 1], crs[:, 0]].astype(np.int64)
    blob = np.repeat(np.arange(n_blobs, dtype=np.int64), sizes)
    span = int(who.max()) + 2 if len(who) else 1
    pair, count = np.unique(blob * span + (who + 1), return_counts=True)
    pair_blob, pair_who = pair // span, pair % span - 1
    unowned = np.zeros(n_blobs, dtype=np.int64)
    unowned[pair_blob[pair_who < 0]] = count[pair_who < 0]
    held = pair_who >= 0
    pair_blob, pair_who, count = pair_blob[held], pair_who[held], count[held]
    n_owners = np.bincount(pair_blob, minlength=n_blobs).astype(np.int64)
    order = np.lexsort((pair_who, -count, pair_blob))      # per blob: most voxels first, then the lowest atom index
    first = order[np.concatenate([[True], np.diff(pair_blob[order]) != 0])] if len(order) else order
    main, main_voxels = np.full(n_blobs, -1, dtype=np.int64), np.zeros(n_blobs, dtype=np.int64)
    main[pair_blob[first]] = pair_who[first]
    main_voxels[pair_blob[first]] = count[first]
    return sizes.astype(np.int64), unowned, n_owners, main, main_voxels


def _norm3(x):
    """np.linalg.norm of a 1-D float64 vector, as numpy computes it (sqrt(x.dot(x))), without the dispatch overhead."""
    return math.sqrt(float(x.dot(x)))


def _crs_keys(crs):
    """Pack raw (c, r, s) triples into sortable int64 keys (21 bits each, offset)."""
    c = np.asarray(crs, dtype=np.int64) + (1 << 20)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def blobDipoleColumns(near, back, greenTotal, redTotal, greenCentroid, redCentroid, ratio):
    """The columns of the dipole table that need no atom, from canned inputs: ``near`` / ``back`` are the ``nearestBlobs`` columns of the green
    list against the red one and of the red list against the green one (``partner``, ``distance``, ``voxelXyz``, ``partnerVoxelXyz``), the
    totals and centroids the two lists' statistics columns.  One row per green blob that has a red partner, in green order: ``green`` / ``red``
    (indices), ``gap`` (A between the two closest voxels), ``mutual`` (the red blob's nearest green blob is this one), ``greenElectrons`` /
    ``redElectrons`` (|total / ratio|), ``balance`` (min / max of the two), ``centroidDistance``, ``midpoint`` (of the two closest voxels) and
    ``shift`` (red centroid -> green centroid: the way the density says the atom should move)."""
    partner = np.asarray(near["partner"], dtype=np.int64)
    green = np.nonzero(partner >= 0)[0].astype(np.int64)
    red = partner[green]
    backPartner = np.asarray(back["partner"], dtype=np.int64)
    greenCentroid, redCentroid = np.asarray(greenCentroid, dtype=np.float64).reshape(-1, 3), np.asarray(redCentroid, dtype=np.float64).reshape(-1, 3)
    greenElectrons = np.abs(np.asarray(greenTotal, dtype=np.float64)[green] / ratio)
    redElectrons = np.abs(np.asarray(redTotal, dtype=np.float64)[red] / ratio)
    with np.errstate(divide="ignore", invalid="ignore"):
        balance = np.minimum(greenElectrons, redElectrons) / np.maximum(greenElectrons, redElectrons)
    shift = greenCentroid[green] - redCentroid[red]
    return {"green": green, "red": red, "gap": np.asarray(near["distance"], dtype=np.float64)[green], "mutual": backPartner[red] == green,
            "greenElectrons": greenElectrons, "redElectrons": redElectrons, "balance": balance, "centroidDistance": np.sqrt((shift ** 2).sum(axis=1)),
            "midpoint": 0.5 * (np.asarray(near["voxelXyz"], dtype=np.float64).reshape(-1, 3)[green] +
                               np.asarray(near["partnerVoxelXyz"], dtype=np.float64).reshape(-1, 3)[green]),
            "shift": shift}


def collinearity(atomXyz, greenCentroid, redCentroid):
    """The cosine at the atom between the directions to the two centroids: -1 = the atom sits between them (NaN when it sits ON one)."""
    u = np.asarray(greenCentroid, dtype=np.float64).reshape(-1, 3) - np.asarray(atomXyz, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(redCentroid, dtype=np.float64).reshape(-1, 3) - np.asarray(atomXyz, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (u * v).sum(axis=1) / np.sqrt((u ** 2).sum(axis=1) * (v ** 2).sum(axis=1))


class DensityAnalysis(object):
    """ref densityAnalysis.py:278-1240 (the accelerated subset)."""

    residueCloudHeader = ['chain', 'residue_number', 'residue_name', 'local_density_electron_ratio', 'num_voxels', 'electrons', 'volume', 'centroid_xyz']
    domainCloudHeader = residueCloudHeader
    blobStatisticsHeader = ['distance_to_atom', 'sign', 'electrons_of_discrepancy', 'num_voxels', 'volume', 'chain', 'residue_number', 'residue_name',
                            'atom_name', 'atom_symmetry', 'atom_xyz', 'centroid_xyz']
    peakStatisticsHeader = ['distance_to_atom', 'sign', 'height_in_sigma', 'height_in_electrons_per_A3', 'blob_index', 'on_border', 'chain', 'residue_number',
                            'residue_name', 'atom_name', 'symmetry', 'atom_xyz', 'peak_xyz']
    basinStatisticsHeader = peakStatisticsHeader + ['num_voxels', 'volume', 'electrons', 'fraction_of_blob', 'saddle_in_sigma', 'prominence_in_sigma', 'neighbour_peak',
                                                    'centroid_xyz']
    blobShapeHeader = ['blob_index', 'num_voxels', 'volume', 'sign', 'electrons_of_discrepancy', 'extreme_in_sigma', 'extreme_in_electrons_per_A3', 'extreme_xyz',
                       'principal_length_1', 'principal_length_2', 'principal_length_3', 'anisotropy', 'box_extent', 'on_border', 'distance_to_atom', 'chain',
                       'residue_number', 'residue_name', 'atom_name', 'atom_symmetry', 'atom_xyz']
    blobDipoleHeader = ['green_index', 'red_index', 'gap_distance', 'mutual', 'green_electrons', 'red_electrons', 'balance', 'centroid_distance', 'midpoint_xyz',
                        'shift_xyz', 'distance_to_atom', 'chain', 'residue_number', 'residue_name', 'atom_name', 'atom_symmetry', 'atom_xyz', 'collinearity']
    regionDensityHeader = ["actual_significant_regional_density", "num_electrons_actual_significant_regional_density"]
    atomRegionDensityHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy"] + regionDensityHeader
    symmetryAtomRegionDensityHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "symmetry", "atom_xyz", "fully_within_density_map"] + regionDensityHeader
    residueRegionDensityHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy"] + regionDensityHeader
    regionDiscrepancyHeader = ["actual_abs_significant_regional_discrepancy", "num_electrons_actual_abs_significant_regional_discrepancy",
                               "expected_abs_significant_regional_discrepancy", "num_electrons_expected_abs_significant_regional_discrepancy",
                               "actual_significant_regional_discrepancy", "num_electrons_actual_significant_regional_discrepancy",
                               "actual_positive_significant_regional_discrepancy", "num_electrons_actual_positive_significant_regional_discrepancy",
                               "actual_negative_significant_regional_discrepancy", "num_electrons_actual_negative_significant_regional_discrepancy"]
    atomRegionDiscrepancyHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy"] + regionDiscrepancyHeader
    symmetryAtomRegionDiscrepancyHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "symmetry", "atom_xyz", "fully_within_density_map"] + regionDiscrepancyHeader
    residueRegionDiscrepancyHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy"] + regionDiscrepancyHeader
    partitionHeader = ['num_voxels', 'positive_discrepancy', 'num_electrons_positive_discrepancy', 'negative_discrepancy', 'num_electrons_negative_discrepancy',
                       'abs_discrepancy', 'num_electrons_abs_discrepancy', 'net_discrepancy', 'num_electrons_net_discrepancy']
    atomPartitionHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy"] + partitionHeader
    residuePartitionHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy"] + partitionHeader
    blobOwnershipHeader = ['num_voxels', 'unowned_voxels', 'num_owner_atoms', 'chain', 'residue_number', 'residue_name', 'atom_name', 'atom_symmetry',
                           'main_owner_voxels']
    atomRadialProfileHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'atom_type', 'electrons', 'bfactor', 'valid',
                               'shell_voxels', 'shell_density', 'shell_significant_voxels', 'shell_significant_density']
    atomTypeRadialProfileHeader = ['atom_type', 'num_atoms', 'optimized_radius', 'shell_outer_radius', 'median_cumulative_density_per_electron', 'profile_radius']
    atomQScoreHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'bfactor', 'valid', 'q_score', 'n_points']
    residueQScoreHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy", 'mean_q_score', 'min_q_score', 'num_atoms_scored']
    atomModelCorrelationHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'bfactor', 'rscc_model', 'rsr_model']
    atomGradientHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'bfactor', 'dT_dx', 'dT_dy', 'dT_dz', 'dT_dB', 'dT_docc',
                          'shift_x', 'shift_y', 'shift_z', 'shift_b', 'shift_occ', 'num_voxels']
    blobFitHeader = ['blob_index', 'blob_num_voxels', 'rank', 'centre', 'rotation', 'score', 'low_atoms', 'rscc', 'xyz']
    refineAtomHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'bfactor', 'refined_x', 'refined_y', 'refined_z', 'refined_bfactor',
                        'refined_occupancy', 'shift', 'delta_b']
    residueModelCorrelationHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy", 'rscc_model', 'rsr_model']
    atomLocalHeader = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", 'bfactor', 'local_cc', 'local_z_diff', 'local_std_diff']
    residueLocalHeader = ['model', 'chain', 'residue_number', 'residue_name', "mean_occupancy", 'mean_local_cc', 'min_local_cc', 'extreme_local_z_diff']

    def __init__(self, pdbid, densityObj=None, diffDensityObj=None, biopdbObj=None, pdbObj=None):
        self.pdbid = pdbid
        self.densityObj = densityObj
        self.diffDensityObj = diffDensityObj
        self.biopdbObj = biopdbObj
        self.pdbObj = pdbObj
        self._symmetryAtoms = None
        self._symmetryOnlyAtoms = None
        self._asymmetryAtoms = None
        self._symmetryAtomCoords = None
        self._symmetryOnlyAtomCoords = None
        self._asymmetryAtomCoords = None
        self._greenBlobList = None
        self._partitions = {}
        self._qScores = None
        self._model = None
        self._modelDifference = None
        self._refined = None
        self._local = {}
        self._redBlobList = None
        self._blueBlobList = None
        self._greenPeakList = None
        self._redPeakList = None
        self._bluePeakList = None
        self._medians = None
        self._atomCloudDescriptions = None
        self._residueCloudDescriptions = None
        self._domainCloudDescriptions = None
        self._densityElectronRatio = None
        self._numVoxelsAggregated = None
        self._totalAggregatedElectrons = None
        self._totalAggregatedDensity = None
        self._atomTypeOverlapCompleteness = None
        self._atomTypeOverlapIncompleteness = None
        self._cloudTables = None
        self._fc = None

    # ---- lazy properties (ref densityAnalysis.py:326-565) ------------------------------------
    def _lazy(name, trigger):
        def getter(self):
            if getattr(self, name) is None:
                getattr(self, trigger)()
            return getattr(self, name)
        return property(getter)

    symmetryAtoms = _lazy('_symmetryAtoms', '_calculateSymmetryAtoms')
    symmetryOnlyAtoms = _lazy('_symmetryOnlyAtoms', '_splitSymmetryAtoms')
    asymmetryAtoms = _lazy('_asymmetryAtoms', '_splitSymmetryAtoms')
    symmetryAtomCoords = _lazy('_symmetryAtomCoords', '_calculateSymmetryAtoms')
    symmetryOnlyAtomCoords = _lazy('_symmetryOnlyAtomCoords', '_splitSymmetryAtoms')
    asymmetryAtomCoords = _lazy('_asymmetryAtomCoords', '_splitSymmetryAtoms')
    medians = _lazy('_medians', 'aggregateCloud')

    def _described(name, which):
        """The description tables (ref densityAnalysis.py:682-731, 734-767) are MADE on first access: aggregateCloud keeps what they
        are made from (numeric columns, row indices) -- `pdb_eda multiple` and the optimiser read the medians and the number of rows,
        never the rows (a 2 000-atom entry spent 0.4 ms of its 1.6 on string columns and lists of Python rows nobody looked at)."""
        def getter(self):
            if getattr(self, name) is None:
                if self._cloudTables is None:
                    self.aggregateCloud()
                if self._cloudTables is not None and getattr(self, name) is None:
                    setattr(self, name, self._cloudTables[which]())
            return getattr(self, name)
        return property(getter)

    atomCloudDescriptions = _described('_atomCloudDescriptions', 'atoms')
    residueCloudDescriptions = _described('_residueCloudDescriptions', 'residues')
    domainCloudDescriptions = _described('_domainCloudDescriptions', 'domains')
    del _described

    @property
    def cloudCounts(self):
        """(atoms, residue clouds, domain clouds) analysed = the lengths of the three description tables, without making them."""
        if self._cloudTables is None:
            self.aggregateCloud()
        return self._cloudTables["counts"] if self._cloudTables is not None else None
    numVoxelsAggregated = _lazy('_numVoxelsAggregated', 'aggregateCloud')
    totalAggregatedElectrons = _lazy('_totalAggregatedElectrons', 'aggregateCloud')
    totalAggregatedDensity = _lazy('_totalAggregatedDensity', 'aggregateCloud')
    densityElectronRatio = _lazy('_densityElectronRatio', 'aggregateCloud')
    atomTypeOverlapCompleteness = _lazy('_atomTypeOverlapCompleteness', 'aggregateCloud')
    atomTypeOverlapIncompleteness = _lazy('_atomTypeOverlapIncompleteness', 'aggregateCloud')
    del _lazy

    def _greenRed(self):
        # ONE fused pass over the Fo-Fc grid gives both lists (the reference thresholds it twice)
        cut = self.diffDensityObj.diffDensityCutoff
        self._greenBlobList, self._redBlobList = self.diffDensityObj.createFullBlobLists(cut)

    @property
    def greenBlobList(self):
        """ref densityAnalysis.py:392-401."""
        if self._greenBlobList is None:
            self._greenRed()
        return self._greenBlobList

    @property
    def redBlobList(self):
        """ref densityAnalysis.py:403-412."""
        if self._redBlobList is None:
            self._greenRed()
        return self._redBlobList

    @property
    def blueBlobList(self):
        """ref densityAnalysis.py:414-423."""
        if self._blueBlobList is None:
            self._blueBlobList = self.densityObj.createFullBlobList(self.densityObj.densityCutoff)
        return self._blueBlobList

    # ---- peak lists (no reference counterpart): local extrema, tied to the blob lists above ----
    def _greenRedPeaks(self):
        # ONE fused pass over the Fo-Fc grid gives both lists; the blob lists at the same cutoff give every peak its blob
        diff = self.diffDensityObj
        self._greenPeakList, self._redPeakList = diff.findPeakLists(diff.diffDensityCutoff, (self.greenBlobList, self.redBlobList))

    @property
    def greenPeakList(self):
        """Maxima of the Fo-Fc map at or above ``diffDensityCutoff`` (3 sigma), strongest first."""
        if self._greenPeakList is None:
            self._greenRedPeaks()
        return self._greenPeakList

    @property
    def redPeakList(self):
        """Minima of the Fo-Fc map at or below ``-diffDensityCutoff``, deepest first."""
        if self._redPeakList is None:
            self._greenRedPeaks()
        return self._redPeakList

    @property
    def bluePeakList(self):
        """Maxima of the 2Fo-Fc map at or above ``densityCutoff``."""
        if self._bluePeakList is None:
            self._bluePeakList = self.densityObj.findPeaks(self.densityObj.densityCutoff, self.blueBlobList)
        return self._bluePeakList

    # ---- aggregateCloud (ref densityAnalysis.py:571-780) --------------------------------------
    def _cloudInputs(self):
        """The arrays of ``pdbeda_cloud_atoms`` for the current parameter tables.  Everything but the radius column depends on
        the structure and on the name -> type / electrons / bonded tables only, so it is kept on the structure's snapshot
        while those tables are the same objects: the iterations of optimise mode (optimizeParams.py:232-243 passes
        ``{**params, "radii": ..., "slopes": ...}``) change radii and slopes, nothing else."""
        cols = _structure.columns(self.biopdbObj)
        tables = (fullAtomNameMapAtomTypeGlobal, fullAtomNameMapElectronsGlobal, bondedAtomsGlobal)
        cached = cols.__dict__.get("_cloud_inputs")
        if cached is None or any(a is not b for a, b in zip(cached[0], tables)):
            cached = (tables, self._cloudInputsFixed(cols))            # (holding the tables keeps their identity meaningful)
            cols._cloud_inputs = cached
        inp = dict(cached[1])
        pair_radius = np.zeros(len(inp["pair_type"]), dtype=np.float32)
        for k in inp["used_pairs"]:
            pair_radius[k] = radiiGlobal[inp["pair_type"][k]]
        inp["radius"] = pair_radius[inp["pair"]]
        return inp

    @staticmethod
    def _cloudInputsFixed(cols, native=None):
        """Flatten what aggregateCloud reads from the structure (densityAnalysis.py:596-603, 617-621, 653-656) into the arrays
        of ``pdbeda_cloud_atoms``: the eligible atoms in the reference's iteration order, a key per (residue, residue_atom
        name), the bonded-name table restricted to each residue, and the 'owners' of the completeness count.  Works on the
        columnar snapshot of the structure (``structure.columns``): no per-atom Python.  The index work is one pass in C
        (``_hostwalk.cloud_inputs``: fifty small numpy calls were 0.3 ms of a 2 000-atom entry) with the numpy form below as
        its fallback and its check (``native``: None = C when built, True / False force one; tests/test_cloud_inputs.py)."""
        names = cols.pair_names
        walk = _structure._hostwalk() if native is not False else None
        if walk is None and native:
            raise ImportError("pdb_eda_amd/_hostwalk.so is not built (python __graft_entry__.py)")
        if walk is not None and hasattr(walk, "cloud_inputs"):
            n_pairs = max(len(names), 1)
            tables = _pairTables(names, n_pairs)
            known = np.zeros(n_pairs, dtype=np.uint8)
            known[:len(names)] = tables["known"]
            out = walk.cloud_inputs(cols.res_of_atom, cols.pair_of_atom, (~cols.res_het).astype(np.uint8), known, cols.occupancy,
                                    np.ascontiguousarray(cols.coord32), tables["nb_off"], tables["nb"])
            sel, residue_of, pair_of, key_of, alias, bonded_off, bonded, owner_key, owner_pair, plain_residues = (
                np.frombuffer(b, dtype=t) for b, t in zip(out, (np.int64, np.int32, np.int64, np.int32, np.int32, np.int64, np.int32, np.int32, np.int64, np.int64)))
            used = np.unique(pair_of)
            electrons = tables["electrons"]
            if len(used) and np.isnan(electrons[used]).any():     # (the reference's electronsMap[name] raises the same KeyError)
                raise KeyError(names[int(used[np.isnan(electrons[used])][0])])
            return {"cols": cols, "rows": sel, "plain_residues": plain_residues, "xyz": cols.coord[sel], "occupancy": cols.occupancy[sel],
                    "electrons": electrons[pair_of], "used_pairs": used.tolist(), "pair": pair_of, "pair_type": tables["pair_type"],
                    "residue": residue_of, "alias": alias, "key": key_of, "bonded_off": bonded_off, "bonded": bonded, "owner_key": owner_key,
                    "owner_type_id": tables["pair_type_id"][owner_pair], "type_names": tables["type_names"], "pair_type_id": tables["pair_type_id"]}
        n_pairs = max(len(names), 1)
        known = _pairTables(names, n_pairs)["known"]
        plain = ~cols.res_het                                                      # residues with id[0] == ' ' (596)
        ordinal = np.cumsum(plain) - 1                                             # their running number
        child = np.nonzero(plain[cols.res_of_atom])[0]                             # EVERY child atom of those residues, in order
        child_res = ordinal[cols.res_of_atom[child]]
        child_pair = cols.pair_of_atom[child]
        eligible = known[child_pair] & (cols.occupancy[child] != 0) if len(child) else np.zeros(0, dtype=bool)
        sel = child[eligible]                                                      # rows of cols.* of the eligible atoms
        residue_of, pair_of = child_res[eligible], child_pair[eligible]
        n = len(sel)
        # key per (residue, name), numbered by first appearance
        code = residue_of * n_pairs + pair_of
        distinct, first, inverse = np.unique(code, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        rank = np.empty(len(distinct), dtype=np.int64)
        rank[by_first] = np.arange(len(distinct))
        key_of = rank[inverse]

        def key_lookup(codes):
            pos = np.minimum(np.searchsorted(distinct, codes), max(len(distinct) - 1, 0))
            found = distinct[pos] == codes if len(distinct) else np.zeros(len(codes), dtype=bool)
            return found, rank[pos[found]]
        # allAtomClouds is keyed by the coordinate: the last atom with the same float32 triple wins (604)
        alias = _lastWithSameCoord(cols.coord32[sel])
        # the pair tables: type, electrons, radius, and the bonded names that exist in this structure
        used = np.unique(pair_of)
        tables = _pairTables(names, n_pairs)
        pair_type, pair_type_id, type_names, nb_off, nb = tables["pair_type"], tables["pair_type_id"], tables["type_names"], tables["nb_off"], tables["nb"]
        pair_electrons = tables["electrons"]
        if len(used) and np.isnan(pair_electrons[used]).any():     # (the reference's electronsMap[name] raises the same KeyError)
            raise KeyError(names[int(used[np.isnan(pair_electrons[used])][0])])
        # bonded keys of every key, in key order then table order
        key_code = distinct[by_first]
        key_res, key_pair = key_code // n_pairs, key_code % n_pairs
        counts = nb_off[key_pair + 1] - nb_off[key_pair]
        owner = np.repeat(np.arange(len(key_code)), counts)
        within = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
        found, bonded = key_lookup(key_res[owner] * n_pairs + nb[nb_off[key_pair][owner] + within]) if len(owner) else (np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64))
        bonded_off = np.concatenate([[0], np.cumsum(np.bincount(owner[found], minlength=len(key_code)))]).astype(np.int64)
        # owners of the completeness count: every child atom whose (residue, name) has a key (653-656)
        found, owner_key = key_lookup(child_res * n_pairs + child_pair)
        return {"cols": cols, "rows": sel, "plain_residues": np.nonzero(plain)[0], "xyz": cols.coord[sel], "occupancy": cols.occupancy[sel],
                "electrons": pair_electrons[pair_of], "used_pairs": used.tolist(), "pair": pair_of, "pair_type": pair_type,
                "residue": residue_of.astype(np.int32), "alias": alias.astype(np.int32), "key": key_of.astype(np.int32),
                "bonded_off": bonded_off, "bonded": bonded.astype(np.int32), "owner_key": owner_key.astype(np.int32),
                "owner_type_id": pair_type_id[child_pair[found]], "type_names": type_names, "pair_type_id": pair_type_id}

    def aggregateCloud(self, minCloudElectrons=25.0, minTotalElectrons=400.0):
        """Aggregate the 2Fo-Fc clouds by atom, residue and domain; sets ``densityElectronRatio``,
        ``medians`` and the description tables.  Same silent-failure contract as the reference
        (Q7): everything stays ``None`` below ``minTotalElectrons`` or if the statistics tail fails.

        Everything that touches voxels -- the clouds of every atom, best cloud and pooling, bonded-atom completeness, the
        residue and domain unions -- is ONE library call (``pdbeda_aggregate_cloud``: voxel lists stay on the device); the
        host flattens the structure into arrays before it and keeps the reference's host-side statistics tail after it."""
        _requireParams()
        densityObj = self.densityObj
        unitVolume = densityObj.header.unitVolume
        typeMap = fullAtomNameMapAtomTypeGlobal
        inp = self._cloudInputs()
        if not len(inp["rows"]):
            return
        res = densityObj._map.aggregate_cloud(inp["xyz"], inp["radius"], inp["electrons"] * inp["occupancy"], inp["residue"], inp["alias"], inp["key"],
                                              inp["bonded_off"], inp["bonded"], inp["owner_key"], densityObj.densityCutoff, minCloudElectrons)
        if not len(res["atom"]):
            return
        completely = collections.defaultdict(int)
        incompletely = collections.defaultdict(int)
        n_types = len(inp["type_names"])
        for counter, state in ((completely, 1), (incompletely, 2)):
            per_type = np.bincount(inp["owner_type_id"][res["owner_state"] == state], minlength=n_types).tolist()
            counter.update({t: c for t, c in zip(inp["type_names"], per_type) if c})
        cols = inp["cols"]
        plain = inp["plain_residues"].tolist()

        def cloudRows(t, by_ratio=False):
            which = [plain[ri] for ri in t["residue"].tolist()]
            rows = [[cols.res_chain[k], cols.res_number[k], cols.res_name[k], tot / el, nv, el, nv * unitVolume, cen]
                    for k, tot, nv, el, cen in zip(which, t["total"].tolist(), t["n"].tolist(), t["electrons"].tolist(), t["centroid"].tolist())]
            if by_ratio:
                rows.sort(key=lambda x: x[3])
            return rows
        numVoxels, totalElectrons, totalDensity = res["numVoxels"], res["totalElectrons"], res["totalDensity"]
        if totalElectrons < minTotalElectrons:
            return
        densityElectronRatio = totalDensity / totalElectrons

        try:
            atoms, n_atoms, medians = self._cloudStatistics(inp, res, densityElectronRatio, unitVolume, typeMap)
        except Exception:
            return
        self._cloudTables = {"atoms": atoms, "residues": lambda: cloudRows(res["res"]), "domains": lambda: cloudRows(res["dom"], True),
                             "counts": (n_atoms, len(res["res"]["n"]), len(res["dom"]["n"]))}
        self._atomCloudDescriptions = self._residueCloudDescriptions = self._domainCloudDescriptions = None

        self._densityElectronRatio = densityElectronRatio
        self._numVoxelsAggregated = numVoxels
        self._totalAggregatedElectrons = totalElectrons
        self._totalAggregatedDensity = totalDensity
        self._medians = medians
        self._atomTypeOverlapCompleteness = completely
        self._atomTypeOverlapIncompleteness = incompletely

    @staticmethod
    def _cloudStatistics(inp, res, ratio, unitVolume, typeMap, native=None):
        """The host-side statistics over the atom table (what densityAnalysis.py:734-767 computes), on whole columns: the
        per-atom-type medians come from ONE sort per column instead of a masked nanmedian per (column, type)."""
        idx = res["atom"]
        dist = res["atom_distance"]
        total, count, centroid = res["atom_total"], res["atom_n"], res["atom_centroid"]
        if not np.isnan(dist).all():
            walk0 = _structure._hostwalk() if native is not False else None
            if walk0 is not None and hasattr(walk0, "nan_cutoff"):                # (numpy's own nanmedian + nanstd * 2, to the bit, without their 0.08 ms of Python)
                near = dist < walk0.nan_cutoff(np.ascontiguousarray(dist, dtype=np.float64), 2.0)
            else:
                near = dist < np.nanmedian(dist) + np.nanstd(dist) * 2          # (the reference filters the finished table: same rows)
            idx, dist, total, count, centroid = idx[near], dist[near], total[near], count[near], centroid[near]
        n = len(idx)
        cols, rows = inp["cols"], inp["rows"][idx]
        of_residue = cols.res_of_atom[rows]
        # atom types as numbers: inp["type_names"] is sorted, so the types present, in np.unique's order, are the ids present
        type_id = inp["pair_type_id"][inp["pair"][idx]]
        present = np.flatnonzero(np.bincount(type_id, minlength=len(inp["type_names"])))
        atom_types = np.asarray(inp["type_names"])[present] if len(present) else np.zeros(0, dtype='U1')
        n_types = len(atom_types)
        group = np.searchsorted(present, type_id)
        # the numeric columns of the atom table (the reference's structured array, 734-741); the table itself -- with its string
        # columns -- is made from them when somebody asks for it (``make_table`` below)
        table = {'density_electron_ratio': total / inp["electrons"][idx] / inp["occupancy"][idx], 'num_voxels': np.asarray(count, dtype=np.int64),
                 'bfactor': np.array(cols.bfactor[rows], dtype=np.float64), 'centroid_distance': np.asarray(dist, dtype=np.float64)}

        def make_table():
            out = np.zeros(n, dtype=np.dtype([
                ('chain', 'U20'), ('residue_number', int), ('residue_name', 'U10'), ('atom_name', 'U10'), ('atom_type', 'U%d' % atomTypeLengthGlobal),
                ('density_electron_ratio', float), ('num_voxels', int), ('electrons', int), ('bfactor', float), ('centroid_distance', float),
                ('centroid_xyz', float, (3,)), ('adj_density_electron_ratio', float), ('domain_fraction', float), ('corrected_fraction', float),
                ('corrected_density_electron_ratio', float), ('volume', float)]))
            out['chain'] = np.asarray(cols.res_chain)[of_residue]
            out['residue_number'] = np.asarray(cols.res_number)[of_residue]
            out['residue_name'] = np.asarray(cols.res_name)[of_residue]
            out['atom_name'] = np.asarray(cols.atom_names)[cols.name_of_atom[rows]] if n else ''
            out['atom_type'] = atom_types[group] if n else ''
            out['electrons'] = inp["electrons"][idx]
            out['centroid_xyz'] = centroid
            for field, values in table.items():
                out[field] = values
            return out

        asDict = lambda per_type: dict(zip(atom_types.tolist(), per_type))     # noqa: E731
        walk = _structure._hostwalk() if native is not False else None
        if walk is None and native:
            raise ImportError("pdb_eda_amd/_hostwalk.so is not built (python __graft_entry__.py)")
        if walk is not None and hasattr(walk, "cloud_stats") and n:
            # the medians, the b-factor regressions and the corrected columns in one pass in C (round 5: ~60 small numpy calls were
            # 0.45 ms of a 2 000-atom entry's 1.3 ms); the numpy form below stays as its fallback and its check (tests/test_structure.py)
            table_slopes = np.array([slopesGlobal[t] for t in atom_types.tolist()], dtype=np.float64)
            rows_b, types_b = walk.cloud_stats(np.ascontiguousarray(group, dtype=np.int64), n_types, np.ascontiguousarray(table['density_electron_ratio'], dtype=np.float64),
                                               table['num_voxels'], table['bfactor'], table['centroid_distance'], table_slopes, float(ratio), float(unitVolume))
            r6 = np.frombuffer(rows_b, dtype=np.float64).reshape(6, n)
            t10 = np.frombuffer(types_b, dtype=np.float64).reshape(10, n_types)
            for k, field in enumerate(('adj_density_electron_ratio', 'bfactor', 'domain_fraction', 'corrected_fraction', 'corrected_density_electron_ratio', 'volume')):
                table[field] = r6[k]
            per_type = dict(zip(('num_voxels', 'volume', 'density_electron_ratio', 'centroid_distance', 'adj_density_electron_ratio', 'bfactor',
                                 'domain_fraction', 'slopes', 'corrected_fraction', 'corrected_density_electron_ratio'), t10))
            medians = {field: asDict(per_type[field]) for field in ('num_voxels', 'density_electron_ratio', 'centroid_distance', 'adj_density_electron_ratio', 'volume',
                                                                    'bfactor', 'slopes', 'domain_fraction', 'corrected_fraction', 'corrected_density_electron_ratio')}
            return make_table, n, medians

        # rows in type order, once: every median below sorts the values of one type at a time, in place
        by_type = np.argsort(group.astype(np.int16 if n_types < 32768 else np.int64), kind="stable")
        start = np.searchsorted(group[by_type], np.arange(n_types + 1))
        runs = list(zip(start[:-1].tolist(), start[1:].tolist()))

        def typeMedians(values, keep=None, also=()):
            """np.nanmedian of ``values`` per atom type (NaNs and dropped rows sort last within a type; the middle one or the mean of
            the middle two of what is left).  ``also``: weakly monotone functions of the values whose per-type medians are wanted as
            well -- the median of f(values) is the mean of f at the same one or two order statistics, so no second sort."""
            v = np.asarray(values, dtype=np.float64)
            if keep is not None:
                v = np.where(keep, v, np.nan)
            sv = v[by_type]
            for lo, hi in runs:
                sv[lo:hi].sort()
            count = np.bincount(group, weights=~np.isnan(v), minlength=n_types).astype(np.int64)
            safe = np.minimum(np.stack([start[:-1] + np.maximum(count - 1, 0) // 2, start[:-1] + count // 2]), max(n - 1, 0))
            middle = sv[safe] if n else np.full((2, n_types), np.nan)
            out = [np.where(count > 0, (f(middle[0]) + f(middle[1])) / 2.0, np.nan) for f in (lambda x: x,) + tuple(also)]
            return out[0] if not also else out

        medians = {}
        m_vox, m_volume = typeMedians(table['num_voxels'], also=(lambda nv: nv * unitVolume,))
        medians['num_voxels'] = asDict(m_vox)
        table['adj_density_electron_ratio'] = table['density_electron_ratio'] / table['num_voxels'] * m_vox[group]
        table['volume'] = table['num_voxels'] * unitVolume
        medians['density_electron_ratio'] = asDict(typeMedians(table['density_electron_ratio']))
        medians['centroid_distance'] = asDict(typeMedians(table['centroid_distance']))
        m_adj, m_fraction = typeMedians(table['adj_density_electron_ratio'], also=(lambda adj: (adj - ratio) / ratio,))
        medians['adj_density_electron_ratio'] = asDict(m_adj)
        medians['volume'] = asDict(m_volume)
        m_b = typeMedians(table['bfactor'], table['bfactor'] > 0)
        medians['bfactor'] = asDict(m_b)
        missing = table['bfactor'] <= 0
        table['bfactor'][missing] = m_b[group][missing]
        # slope of the b-factor dependence per atom type: linear regression where there is something to fit, else the table's slope
        fraction = (table['adj_density_electron_ratio'] - ratio) / ratio
        log_b = np.log(table['bfactor'])
        fit_slope, fit_p, fitted = _typeRegressions(log_b, fraction, table['bfactor'], group, n_types)
        table_slopes = np.array([slopesGlobal[t] for t in atom_types.tolist()], dtype=np.float64)
        slopes = np.where(fitted & ~(fit_p > 0.05), fit_slope, table_slopes)
        medians['slopes'] = asDict(slopes)
        table['domain_fraction'] = fraction
        table['corrected_fraction'] = fraction - (log_b - np.log(m_b[group])) * slopes[group]
        table['corrected_density_electron_ratio'] = table['corrected_fraction'] * ratio + ratio
        medians['domain_fraction'] = asDict(m_fraction)
        m_corrected, m_corrected_ratio = typeMedians(table['corrected_fraction'], also=(lambda c: c * ratio + ratio,))
        medians['corrected_fraction'] = asDict(m_corrected)
        medians['corrected_density_electron_ratio'] = asDict(m_corrected_ratio)
        return make_table, n, medians

    # ---- symmetry atoms (ref densityAnalysis.py:885-912 + cutils.pyx:73-103) -------------------
    def _calculateSymmetryAtoms(self):
        densityObj = self.densityObj
        header = densityObj.header
        ncrs = header.ncrs
        corners = np.array([[c, r, s] for c in [0, ncrs[0] - 1] for r in [0, ncrs[1] - 1] for s in [0, ncrs[2] - 1]], dtype=np.int32)
        box = densityObj._map.crs2xyz(corners)
        lo, hi = box.min(axis=0), box.max(axis=0)
        cols = _structure.columns(self.biopdbObj)
        coords = cols.coord
        rot = np.array([np.asarray(m, dtype=np.float64) for m in self.pdbObj.header.rotationMats])
        idx, sym, xyz = densityObj._ctx.symmetry_atoms(coords, rot, np.asarray(header.orthoMat, dtype=np.float64), lo, hi)
        ident = ~np.any(sym != 0, axis=1)
        allCoords = np.where(ident[:, None], coords[idx], xyz)      # == np.asarray([atom.coord ...]): float32 coordinates promote exactly
        # the SymAtom objects are made on demand: a blob-statistics table touches a few hundred of the thousands there are
        allAtoms = _SymAtomList(cols, idx, sym, xyz, ident)
        self._symmetryAtoms = allAtoms
        self._symmetryAtomCoords = allCoords
        self._symmetryOnlyAtoms = self._asymmetryAtoms = self._symmetryOnlyAtomCoords = self._asymmetryAtomCoords = None

    def _splitSymmetryAtoms(self):
        """The symmetry-only / asymmetric-unit halves of the list (ref densityAnalysis.py:905-912), made when somebody asks for them: the blob
        statistics read the whole list only."""
        allAtoms, allCoords = self.symmetryAtoms, self.symmetryAtomCoords
        ident = allAtoms._ident
        self._symmetryOnlyAtoms = allAtoms.subset(np.nonzero(~ident)[0])
        self._symmetryOnlyAtomCoords = allCoords[~ident]
        self._asymmetryAtoms = allAtoms.subset(np.nonzero(ident)[0])
        self._asymmetryAtomCoords = allCoords[ident]

    # ---- blob statistics (ref densityAnalysis.py:914-939) --------------------------------------
    def calculateAtomSpecificBlobStatistics(self, blobList):
        symmetryAtoms = self.symmetryAtoms
        symmetryAtomCoords = self.symmetryAtomCoords
        if not self.densityElectronRatio:
            raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
        ratio = self.densityElectronRatio
        if not blobList:
            return []
        if len(symmetryAtomCoords) == 0:
            # no symmetry atoms (a file without REMARK 290 has no operators): the reference's cdist() of a centroid against an
            # empty coordinate array raises this ValueError (densityAnalysis.py:933) -- an ordinary per-entry failure, not a device error
            raise ValueError("XB must be a 2-dimensional array.")
        listed = blobList.columns() if isinstance(blobList, ccp4.DeviceBlobs) else None
        if listed is not None:                   # straight from the device list's columns: no blob object is made for the table
            centroid_xyz = np.ascontiguousarray(listed["centroid"], dtype=np.float64)
            centroid = centroid_xyz                                  # (n x 3: _rows makes a list of three floats per row)
            total = listed["totalDensity"]
            num_voxels, volume = np.asarray(listed["n"], dtype=np.int64), np.asarray(listed["volume"], dtype=np.float64)
        else:
            centroid = [blob.centroid for blob in blobList]
            centroid_xyz = np.array(centroid, dtype=np.float64)
            total = np.array([blob.totalDensity for blob in blobList], dtype=np.float64)
            num_voxels, volume = [blob.numVoxels for blob in blobList], [blob.volume for blob in blobList]
        idx, dist = self.densityObj._ctx.nearest_atom(centroid_xyz, np.asarray(symmetryAtomCoords, dtype=np.float64))
        rows, symmetry, coords = symmetryAtoms.columns(idx)
        cols = _structure.columns(self.biopdbObj)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        chain, number, resname = (cols.atom_lists(which) for which in ("chain", "number", "resname"))
        sign = np.where(total >= 0, '+', '-').tolist()
        return self._rows(list(dist), sign, np.abs(total / ratio), num_voxels, volume,
                          (chain, rows), (number, rows), (resname, rows), (cols.name if isinstance(cols.name, (list, tuple)) else list(cols.name), rows),       # (picked by _rows)
                          symmetry, coords, centroid)

    # ---- peak statistics (no reference counterpart; built like the blob table above) ------------
    def calculateAtomSpecificPeakStatistics(self, peakList):
        """One row per peak (``peakStatisticsHeader``): the nearest symmetry atom is taken from the REFINED peak position;
        height in units of the map's standard deviation and in electrons per cubic Angstrom (height / densityElectronRatio)."""
        symmetryAtoms = self.symmetryAtoms
        symmetryAtomCoords = self.symmetryAtomCoords
        if not self.densityElectronRatio:
            raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
        ratio = self.densityElectronRatio
        if not peakList:
            return []
        if len(symmetryAtomCoords) == 0:
            raise ValueError("XB must be a 2-dimensional array.")       # (the blob table's failure for a file without operators)
        if isinstance(peakList, ccp4.DevicePeaks):
            listed, std = peakList.columns(), peakList.densityMatrix.stdDensity
            peak_xyz = np.ascontiguousarray(listed["xyz"], dtype=np.float64)
            height = np.asarray(listed["height"], dtype=np.float64)
            blob, border = np.asarray(listed["blobIndex"], dtype=np.int64), np.asarray(listed["onBorder"], dtype=np.bool_)
        else:
            std = peakList[0].densityMatrix.stdDensity
            peak_xyz = np.array([peak.xyz for peak in peakList], dtype=np.float64)
            height = np.array([peak.height for peak in peakList], dtype=np.float64)
            blob = np.array([peak.blobIndex for peak in peakList], dtype=np.int64)
            border = np.array([peak.onBorder for peak in peakList], dtype=np.bool_)
        idx, dist = self.densityObj._ctx.nearest_atom(peak_xyz, np.asarray(symmetryAtomCoords, dtype=np.float64))
        rows, symmetry, coords = symmetryAtoms.columns(idx)
        cols = _structure.columns(self.biopdbObj)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        chain, number, resname = (cols.atom_lists(which) for which in ("chain", "number", "resname"))
        sign = np.where(height >= 0, '+', '-').tolist()
        return self._rows(list(dist), sign, height / std, height / ratio, blob, border,
                          (chain, rows), (number, rows), (resname, rows), (cols.name if isinstance(cols.name, (list, tuple)) else list(cols.name), rows),
                          symmetry, coords, peak_xyz)

    # ---- basin statistics (no reference counterpart): the peak table, with what belongs to each peak ----
    def calculateAtomSpecificBasinStatistics(self, peakList):
        """One row per peak of a device list (``basinStatisticsHeader``): the peak table's columns, then the peak's basin -- voxels, volume,
        electrons (|sum / densityElectronRatio|), its share of the blob's density (None when the search was given no blob list), the pass to
        the adjacent basin and the prominence in units of the map's standard deviation, the peak beyond the pass (-1: the basin is its
        whole blob) and the density-weighted centre."""
        shared = self.calculateAtomSpecificPeakStatistics(peakList)          # (raises the blob table's RuntimeError without a ratio)
        if not shared:
            return []
        if not isinstance(peakList, ccp4.DevicePeaks):
            raise ValueError("basin statistics need the peak list findPeaks / findPeakLists returned")
        ratio, std = self.densityElectronRatio, peakList.densityMatrix.stdDensity
        basins, listed = peakList.basinColumns(), peakList.columns()
        total = np.asarray(basins["totalDensity"], dtype=np.float64)
        fraction = [None] * len(total)
        if peakList.blobList is not None:
            blobTotal = np.asarray(peakList.blobList.columns()["totalDensity"], dtype=np.float64)
            blob = np.asarray(listed["blobIndex"], dtype=np.int64)
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.abs(total) / np.abs(blobTotal[np.maximum(blob, 0)])
            fraction = [float(v) if b >= 0 else None for v, b in zip(share.tolist(), blob.tolist())]
        extra = zip(basins["numVoxels"].tolist(), basins["volume"].tolist(), np.abs(total / ratio).tolist(), fraction,
                    (basins["saddle"].astype(np.float64) / std).tolist(), (basins["prominence"] / std).tolist(), basins["neighbour"].tolist(),
                    basins["centroid"].tolist())
        return [list(row) + list(more) for row, more in zip(shared, extra)]

    # ---- blob shape statistics (no reference counterpart; built like the two tables above) ------
    def calculateBlobShapeStatistics(self, blobList):
        """One row per blob of a device list (``blobShapeHeader``): size, total density, the extreme voxel (in units of the map's standard deviation
        and in electrons per cubic Angstrom), the principal RMS lengths in A, the anisotropy 1 - l3 / l1, the box extent along the map axes,
        whether the box touches the non-repeating box, and the symmetry atom nearest to the EXTREME voxel."""
        symmetryAtoms = self.symmetryAtoms
        symmetryAtomCoords = self.symmetryAtomCoords
        if not self.densityElectronRatio:
            raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
        ratio = self.densityElectronRatio
        if not isinstance(blobList, ccp4.DeviceBlobs):
            raise ValueError("blobList must be what createFullBlobList / findAberrantBlobs / createBlobList returned")
        if not blobList:
            return []
        if len(symmetryAtomCoords) == 0:
            raise ValueError("XB must be a 2-dimensional array.")       # (the blob table's failure for a file without operators)
        shape = blobList.shapeColumns()
        segments = blobList._segments
        num_voxels, volume, total = (np.concatenate([np.asarray(seg.stats[k]) for seg in segments]) for k in ("n", "volume", "totalDensity"))
        std = np.concatenate([np.full(len(seg), seg.densityMatrix.stdDensity) for seg in segments])
        extreme = np.asarray(shape["extremeDensity"], dtype=np.float64)
        extreme_xyz = np.ascontiguousarray(shape["extremeXyz"], dtype=np.float64)
        idx, dist = self.densityObj._ctx.nearest_atom(extreme_xyz, np.asarray(symmetryAtomCoords, dtype=np.float64))
        rows, symmetry, coords = symmetryAtoms.columns(idx)
        cols = _structure.columns(self.biopdbObj)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        chain, number, resname = (cols.atom_lists(which) for which in ("chain", "number", "resname"))
        lengths = np.asarray(shape["principalLengths"], dtype=np.float64)
        sign = np.where(total >= 0, '+', '-').tolist()
        return self._rows(np.arange(len(num_voxels), dtype=np.int64), np.asarray(num_voxels, dtype=np.int64), np.asarray(volume, dtype=np.float64), sign,
                          np.abs(total / ratio), extreme / std, extreme / ratio, extreme_xyz, np.ascontiguousarray(lengths[:, 0]), np.ascontiguousarray(lengths[:, 1]),
                          np.ascontiguousarray(lengths[:, 2]), np.asarray(shape["anisotropy"], dtype=np.float64), np.ascontiguousarray(shape["boxExtent"], dtype=np.float64),
                          np.asarray(shape["onBorder"], dtype=np.bool_), list(dist),
                          (chain, rows), (number, rows), (resname, rows), (cols.name if isinstance(cols.name, (list, tuple)) else list(cols.name), rows),
                          symmetry, coords)

    # ---- green / red dipoles (no reference counterpart; built like the tables above) ------------
    def calculateBlobDipoles(self, greenBlobs, redBlobs, maxDistance=2.5):
        """One row (``blobDipoleHeader``) per green blob that has a red blob within ``maxDistance`` A of one of its voxels, in green order: the two
        indices, the gap between the two closest voxels, ``mutual`` (the red blob's nearest green blob is this one: a second device call with the
        lists swapped), the electrons of each blob and their balance min / max, the distance of the centroids, the midpoint of the two closest
        voxels, the shift vector from the red centroid to the green one, the symmetry atom nearest to that midpoint and ``collinearity``: the cosine
        at that atom between the directions to the two centroids (-1: the atom sits between them -- it is in the wrong place by about the shift).
        The default of 2.5 A is a choice (about one atom diameter), not a measured optimum.  Totals and centroids are the device lists' own
        columns (as in the shape table): blob objects of these lists that somebody has changed since (``merge``) are not looked at."""
        symmetryAtoms = self.symmetryAtoms
        symmetryAtomCoords = self.symmetryAtomCoords
        if not self.densityElectronRatio:
            raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
        ratio = self.densityElectronRatio
        if not isinstance(greenBlobs, ccp4.DeviceBlobs) or not isinstance(redBlobs, ccp4.DeviceBlobs):
            raise ValueError("greenBlobs and redBlobs must be what createFullBlobLists / createFullBlobList returned")
        near = greenBlobs.nearestBlobs(redBlobs, maxDistance)                # (ValueError for joined or non-whole-map lists)
        if not (near["partner"] >= 0).any():
            return []
        if len(symmetryAtomCoords) == 0:
            raise ValueError("XB must be a 2-dimensional array.")       # (the blob table's failure for a file without operators)
        back = redBlobs.nearestBlobs(greenBlobs, maxDistance)
        greenStats, redStats = greenBlobs._segments[0].stats, redBlobs._segments[0].stats
        d = blobDipoleColumns(near, back, greenStats["totalDensity"], redStats["totalDensity"], greenStats["centroid"], redStats["centroid"], ratio)
        midpoint = np.ascontiguousarray(d["midpoint"], dtype=np.float64)
        idx, dist = self.densityObj._ctx.nearest_atom(midpoint, np.asarray(symmetryAtomCoords, dtype=np.float64))
        rows, symmetry, coords = symmetryAtoms.columns(idx)
        cols = _structure.columns(self.biopdbObj)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        chain, number, resname = (cols.atom_lists(which) for which in ("chain", "number", "resname"))
        atom_xyz = np.asarray(symmetryAtomCoords, dtype=np.float64)[np.asarray(idx, dtype=np.int64)]
        cosine = collinearity(atom_xyz, np.asarray(greenStats["centroid"])[d["green"]], np.asarray(redStats["centroid"])[d["red"]])
        return self._rows(d["green"], d["red"], np.ascontiguousarray(d["gap"]), np.ascontiguousarray(d["mutual"], dtype=np.bool_), d["greenElectrons"], d["redElectrons"],
                          d["balance"], d["centroidDistance"], midpoint, np.ascontiguousarray(d["shift"], dtype=np.float64), list(dist),
                          (chain, rows), (number, rows), (resname, rows), (cols.name if isinstance(cols.name, (list, tuple)) else list(cols.name), rows),
                          symmetry, coords, np.ascontiguousarray(cosine))

    # ---- Fo / Fc maps, RSCC / RSR (ref densityAnalysis.py:426-446, 783-882) -------------------
    @property
    def fo(self):
        """ref densityAnalysis.py:438-446: the Fo map is the 2Fo-Fc map."""
        return self.densityObj

    @property
    def fc(self):
        """ref densityAnalysis.py:426-435: Fc = 2Fo-Fc - 2 (Fo-Fc), as a DensityMatrix.

        Reference behaviour kept on purpose: the reference makes a ``deepcopy`` of the 2Fo-Fc object and replaces only
        ``.density`` -- ``densityArray`` and the cached ``meanDensity`` / ``stdDensity`` / ``getTotalAbsDensity`` stay those
        of the Fo map (golden ``fc_mean_std``).  The grid is computed on the device (``pdbeda_map_combine``) and stored as
        float32 (the reference's is float64):
        the metrics below therefore take Fc voxel values as ``fo - 2 * diff`` in float64 from the two gathered float32
        values, which is exact."""
        if self._fc is None:
            d = self.densityObj
            fc = ccp4.DensityMatrix.fromDeviceMap(d.header, d.origin, type(d._map).combine(d._map, self.diffDensityObj._map, -2.0), d.pdbid, d._ctx)
            fc._flatOf = d                      # (== fc.densityArray = d.densityArray, without fetching a host copy)
            fc._meanDensity, fc._stdDensity = d.meanDensity, d.stdDensity
            fc._totalAbsDensity = d._totalAbsDensity
            self._fc = fc
        return self._fc

    def medianAbsFoFc(self):
        """ref densityAnalysis.py:783-801: medians of |Fo| and |Fc| over the voxels of the unique box whose |Fo| and |Fc| are
        both below mean + 1 sigma (the Fc statistics are those of Fo: see ``fc``).  Exact order statistics by a device-side
        radix select (``pdbeda_abs_select_hist``): the maps do not move; Fc values are fo - 2 diff in float64 like the reference's."""
        fo, fc = self.fo, self.fc
        foCut = fo.meanDensity + 1.0 * fo.stdDensity
        fcCut = fc.meanDensity + 1.0 * fc.stdDensity
        a, b = fo._map, self.diffDensityObj._map
        n = a.abs_order_statistics(b, -2.0, foCut, fcCut, 0)
        if n == 0:
            return (float("nan"), float("nan"))
        ranks = [n // 2] if n % 2 else [n // 2 - 1, n // 2]
        return tuple(float(np.mean(a.abs_order_statistics(b, -2.0, foCut, fcCut, which, ranks))) for which in (0, 1))

    residueMetricsHeaderList = ['chain', 'residue_number', 'residue_name', "rscc", "rsr", "mean_occupancy", "occupancy_weighted_mean_bfactor"]
    atomMetricsHeaderList = ['chain', 'residue_number', 'residue_name', "atom_name", "symmetry", "xyz", "rscc", "rsr", "occupancy", "bfactor"]

    def _metricsRadius(self):
        """ref densityAnalysis.py:813-818 / 850-855."""
        resolution = self.biopdbObj.header['resolution']
        radius = 0.7
        if 0.6 <= resolution <= 3:
            radius = (resolution - 0.6) / 3 + 0.7
        elif resolution > 3:
            radius = resolution * 0.5
        return radius

    def _rsccRsr(self, groups, radius):
        """RSCC and RSR of every group of coordinates: ONE sphere batch (all voxels of the sphere union, de-duplicated on the
        raw crs like the reference's set), two gathers (2Fo-Fc and Fo-Fc values under the wrap contract), then segmented
        float64 sums.  Pearson r as scipy.stats.pearsonr computes it (centre, normalise, dot, clip)."""
        return self._groupCorrelations(groups, radius, lambda crs, fo: fo - self.diffDensityObj._map.point_density(crs) * 2)

    def _groupCorrelations(self, groups, radius, calculated):
        """``_rsccRsr`` for any calculated map: ``calculated(crs, fo)`` gives its values at the gathered voxels."""
        xyz = np.array([c for g in groups for c in g], dtype=np.float64).reshape(-1, 3)
        off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
        bl = self.densityObj._map.sphere_blobs(xyz, np.full(len(xyz), radius, dtype=np.float32), off, 0.0)
        st = bl.stats()
        crs, voff = bl.voxels()
        vgroup = np.repeat(st["group"].astype(np.int64), np.diff(voff))
        order = np.argsort(vgroup, kind="stable")
        crs, vgroup = crs[order], vgroup[order]
        fo = self.densityObj._map.point_density(crs)
        fc = calculated(crs, fo)
        n_groups = len(groups)
        cnt = np.bincount(vgroup, minlength=n_groups).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        rscc = np.full(n_groups, np.nan)
        rsr = np.full(n_groups, np.nan)
        has = cnt > 0
        if has.any():
            seg = start[has]
            mean_fo = np.add.reduceat(fo, seg) / cnt[has]
            mean_fc = np.add.reduceat(fc, seg) / cnt[has]
            idx = np.cumsum(has) - 1                       # group -> row of the non-empty tables
            xm = fo - mean_fo[idx[vgroup]]
            ym = fc - mean_fc[idx[vgroup]]
            nx = np.sqrt(np.add.reduceat(xm * xm, seg))
            ny = np.sqrt(np.add.reduceat(ym * ym, seg))
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.add.reduceat((xm / nx[idx[vgroup]]) * (ym / ny[idx[vgroup]]), seg)
                rscc[has] = np.clip(r, -1.0, 1.0)
                rsr[has] = np.add.reduceat(np.abs(fo - fc), seg) / np.add.reduceat(np.abs(fo + fc), seg)
            rscc[cnt < 2] = np.nan                          # scipy raises for fewer than two points
        return rscc, rsr

    def calculateRsccRsrMetrics(self, crsList):
        """ref densityAnalysis.py:864-882 for one explicit voxel set."""
        crs = np.asarray(sorted(set(map(tuple, crsList))), dtype=np.int32).reshape(-1, 3)
        fo = self.densityObj._map.point_density(crs)
        fc = fo - self.diffDensityObj._map.point_density(crs) * 2
        xm, ym = fo - fo.mean(), fc - fc.mean()
        rscc = float(np.clip(np.dot(xm / np.linalg.norm(xm), ym / np.linalg.norm(ym)), -1.0, 1.0)) if len(crs) > 1 else float("nan")
        rsr = float(np.abs(fo - fc).sum() / np.abs(fo + fc).sum())
        return (rscc, rsr)

    def residueMetrics(self, residueList=None):
        """ref densityAnalysis.py:803-838: [chain, resnum, resname, rscc, rsr, mean occupancy, occupancy-weighted mean B]."""
        radius = self._metricsRadius()
        if residueList is None:
            residueList = list(self.biopdbObj.get_residues())
        rscc, rsr = self._rsccRsr([[atom.coord for atom in residue.child_list] for residue in residueList], radius)
        results = []
        for residue, cc, rr in zip(residueList, rscc, rsr):
            bfactorWeightedSum = occupancySum = 0.0
            for atom in residue.child_list:
                bfactorWeightedSum += atom.get_bfactor() * atom.get_occupancy()
                occupancySum += atom.get_occupancy()
            results.append([residue.parent.id, residue.id[1], residue.resname, float(cc), float(rr), occupancySum / len(residue.child_list),
                            bfactorWeightedSum / occupancySum])
        return results

    def atomMetrics(self, atomList=None):
        """ref densityAnalysis.py:840-862: [chain, resnum, resname, atom, symmetry, xyz, rscc, rsr, occupancy, bfactor]."""
        radius = self._metricsRadius()
        if atomList is None:
            atomList = self.asymmetryAtoms
        rscc, rsr = self._rsccRsr([[atom.coord] for atom in atomList], radius)
        return [[atom.parent.parent.id, atom.parent.id[1], atom.parent.resname, atom.name, atom.symmetry, atom.coord, float(cc), float(rr),
                 atom.get_occupancy(), atom.get_bfactor()] for atom, cc, rr in zip(atomList, rscc, rsr)]

    # ---- region density / discrepancy (ref densityAnalysis.py:948-1211), batched ---------------
    @staticmethod
    def _flatten(groups, radii):
        """Lists of coordinate lists + per-coordinate radius lists -> (xyz[n, 3], radius[n], offsets[groups + 1])."""
        sizes = np.fromiter((len(g) for g in groups), dtype=np.int64, count=len(groups))
        xyz = np.array([c for g in groups for c in g], dtype=np.float64).reshape(-1, 3)
        rad = np.fromiter((r for g in radii for r in g), dtype=np.float32, count=int(sizes.sum()))
        return xyz, rad, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    def _needRatio(self):
        if not self.densityElectronRatio:
            raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
        return self.densityElectronRatio

    def _densityColumns(self, xyz, rad, off, numSD):
        """The two columns of regionDensityHeader for every group of spheres (ONE device batch), and the validity flags."""
        ratio = self._needRatio()
        dm = self.densityObj
        pos, neg, cnt, valid = dm._map.region_sums(xyz, rad, off, dm.meanDensity + numSD * dm.stdDensity)
        return [pos, pos / ratio], valid

    def _discrepancyColumns(self, xyz, rad, off, numSD):
        """The ten columns of regionDiscrepancyHeader for every group, computed on whole columns (densityAnalysis.py:1200-1211)."""
        ratio = self._needRatio()
        dm = self.diffDensityObj
        cutoff = dm.meanDensity + numSD * dm.stdDensity
        pos, neg, cnt, valid = dm._map.region_sums(xyz, rad, off, cutoff)
        avg = dm.getTotalAbsDensity(cutoff) / dm.numStoredVoxels
        absd = np.abs(pos) + np.abs(neg)
        expected = avg * cnt
        net = pos + neg
        return [absd, absd / ratio, expected, expected / ratio, net, net / ratio, pos, pos / ratio, neg, neg / ratio], valid      # (whole columns: _rows makes the Python numbers)

    @staticmethod
    def _rows(*columns):
        """The table rows (lists) of whole columns: lists, numpy arrays (their ``.tolist()`` values; a 2-D array of ints gives a TUPLE per row), or
        (list, int64 index array) picks.
        One pass in C (``_hostwalk.table_rows``) when the helper is built; ``list(map(list, zip(...)))`` over plain lists otherwise."""
        walk = _structure._hostwalk()
        if walk is not None and hasattr(walk, "table_rows") and 1 <= len(columns) <= 32:
            prepared = [np.ascontiguousarray(c) if isinstance(c, np.ndarray) else c for c in columns]
            if all(not isinstance(c, np.ndarray) or ((c.ndim == 1 and c.dtype in (np.float64, np.int64, np.int32, np.bool_)) or (c.ndim == 2 and c.dtype in (np.float64, np.int64)))
                   for c in prepared):
                return walk.table_rows(prepared)
        plain = []
        for c in columns:
            if isinstance(c, tuple) and len(c) == 2 and isinstance(c[1], np.ndarray):
                plain.append([c[0][r] for r in c[1].tolist()])
            elif isinstance(c, np.ndarray) and c.ndim == 2 and c.dtype.kind in "iu":
                plain.append(list(map(tuple, c.tolist())))                     # (rows of ints are tuples: the symmetry operators)
            else:
                plain.append(c.tolist() if isinstance(c, np.ndarray) else c)
        return list(map(list, zip(*plain)))

    def _atomPick(self, type):
        """Rows of the structure columns of the atoms named ``type`` (all when empty) and their leading table columns (model,
        chain, residue number, residue name, atom name, occupancy: densityAnalysis.py:966-971)."""
        cols = _structure.columns(self.biopdbObj)
        lead = [cols.atom_lists("model"), cols.atom_lists("chain"), cols.atom_lists("number"), cols.atom_lists("resname"), cols.name, cols.occupancy_raw]
        if not type:
            return cols, np.arange(len(cols.atoms)), lead
        pick = np.nonzero(np.asarray(cols.name) == type)[0] if cols.atoms else np.zeros(0, dtype=np.int64)
        rows = pick.tolist()
        return cols, pick, [[column[r] for r in rows] for column in lead]

    def _pairRadius(self, cols, radius, useOptimizedRadii):
        """Per-atom radius of the structure columns: the optimised radius of the atom type where the name is known, else ``radius``."""
        if not useOptimizedRadii:
            return np.full(len(cols.atoms), radius, dtype=np.float32)
        typeMap = fullAtomNameMapAtomTypeGlobal
        per_pair = np.array([radiiGlobal[typeMap[name]] if name in typeMap else radius for name in cols.pair_names] + [radius], dtype=np.float32)
        return per_pair[cols.pair_of_atom]

    def _symmetryPick(self, type):
        atom_rows, symmetry, coords = self.symmetryAtoms.columns(None, type)
        cols = _structure.columns(self.biopdbObj)
        rows = atom_rows.tolist()
        lead = [[column[r] for r in rows] for column in (cols.atom_lists("model"), cols.atom_lists("chain"), cols.atom_lists("number"), cols.atom_lists("resname"), cols.name)]
        xyz = np.array(coords, dtype=np.float64).reshape(-1, 3)
        return cols, atom_rows, lead + [symmetry, coords], xyz

    def _residuePick(self, type, keepAtom, dropEmpty):
        """Residues (optionally only those named ``type``) with the atoms ``keepAtom(residue name, atom name)`` lets through:
        (lead columns incl. the mean occupancy, atom rows, offsets)."""
        cols = _structure.columns(self.biopdbObj)
        n_res = len(cols.residues)
        res_keep = np.ones(n_res, dtype=bool) if not type else np.asarray(cols.res_name) == type
        atom_keep = res_keep[cols.res_of_atom] if len(cols.atoms) else np.zeros(0, dtype=bool)
        if keepAtom is not None:
            resname = cols.atom_lists("resname")
            atom_keep = atom_keep & np.fromiter((keepAtom(rn, an) for rn, an in zip(resname, cols.name)), dtype=bool, count=len(cols.atoms))
        counts = np.bincount(cols.res_of_atom[atom_keep], minlength=n_res) if len(cols.atoms) else np.zeros(n_res, dtype=np.int64)
        if dropEmpty:
            res_keep = res_keep & (counts > 0)
        which = np.nonzero(res_keep)[0]
        counts = counts[which]
        atom_rows = np.nonzero(atom_keep)[0]
        mean_occupancy = _segmentMeans(cols.occupancy[atom_rows], counts)
        rows = which.tolist()
        lead = [[column[r] for r in rows] for column in (cols.res_model, cols.res_chain, cols.res_number, cols.res_name)] + [list(mean_occupancy)]
        return cols, lead, atom_rows, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    def calculateRegionDensity(self, xyzCoordList, radius, numSD=1.5, testValidCrs=False):
        """ref densityAnalysis.py:1037-1068."""
        rad = list(radius) if isinstance(radius, (list, tuple, np.ndarray)) else [radius] * len(xyzCoordList)
        columns, valid = self._densityColumns(*self._flatten([list(xyzCoordList)], [rad]), numSD)
        row = [column.tolist()[0] for column in columns]
        return (row, bool(valid[0])) if testValidCrs else row

    def calculateRegionDiscrepancy(self, xyzCoordList, radius, numSD=3.0, testValidCrs=False):
        """ref densityAnalysis.py:1160-1211."""
        rad = list(radius) if isinstance(radius, (list, tuple, np.ndarray)) else [radius] * len(xyzCoordList)
        columns, valid = self._discrepancyColumns(*self._flatten([list(xyzCoordList)], [rad]), numSD)
        row = [column.tolist()[0] for column in columns]
        return (row, bool(valid[0])) if testValidCrs else row

    def calculateAtomRegionDensity(self, radius, numSD=1.5, type="", useOptimizedRadii=False):
        """ref densityAnalysis.py:948-973 (all atoms in ONE device batch)."""
        cols, pick, lead = self._atomPick(type)
        columns, _ = self._densityColumns(cols.coord[pick], self._pairRadius(cols, radius, useOptimizedRadii)[pick], np.arange(len(pick) + 1, dtype=np.int64), numSD)
        return self._rows(*lead, *columns)

    def calculateSymmetryAtomRegionDensity(self, radius, numSD=1.5, type="", useOptimizedRadii=False):
        """ref densityAnalysis.py:975-999."""
        cols, atom_rows, lead, xyz = self._symmetryPick(type)
        columns, valid = self._densityColumns(xyz, self._pairRadius(cols, radius, useOptimizedRadii)[atom_rows], np.arange(len(atom_rows) + 1, dtype=np.int64), numSD)
        return self._rows(*lead, valid.astype(bool), *columns)

    def calculateResidueRegionDensity(self, radius, numSD=1.5, type="", atomMask=None, useOptimizedRadii=False):
        """ref densityAnalysis.py:1001-1035 (residues left without atoms by the mask are skipped)."""
        keep = None if not atomMask else (lambda resname, name: resname not in atomMask or name in atomMask[resname])
        cols, lead, atom_rows, off = self._residuePick(type, keep, True)
        columns, _ = self._densityColumns(cols.coord[atom_rows], self._pairRadius(cols, radius, useOptimizedRadii)[atom_rows], off, numSD)
        return self._rows(*lead, *columns)

    def calculateAtomRegionDiscrepancies(self, radius, numSD=3.0, type=""):
        """ref densityAnalysis.py:1081-1104 (33 ms/atom in the reference; ONE device batch here)."""
        cols, pick, lead = self._atomPick(type)
        columns, _ = self._discrepancyColumns(cols.coord[pick], np.full(len(pick), radius, dtype=np.float32), np.arange(len(pick) + 1, dtype=np.int64), numSD)
        return self._rows(*lead, *columns)

    def calculateSymmetryAtomRegionDiscrepancies(self, radius, numSD=3.0, type=""):
        """ref densityAnalysis.py:1106-1128."""
        cols, atom_rows, lead, xyz = self._symmetryPick(type)
        columns, valid = self._discrepancyColumns(xyz, np.full(len(atom_rows), radius, dtype=np.float32), np.arange(len(atom_rows) + 1, dtype=np.int64), numSD)
        return self._rows(*lead, valid.astype(bool), *columns)

    def calculateResidueRegionDiscrepancies(self, radius, numSD=3.0, type="", atomMask=None):
        """ref densityAnalysis.py:1130-1158 (with a mask, only atoms the mask names; residues it empties stay in the table)."""
        keep = None if not atomMask else (lambda resname, name: resname in atomMask and name in atomMask[resname])
        cols, lead, atom_rows, off = self._residuePick(type, keep, False)
        columns, _ = self._discrepancyColumns(cols.coord[atom_rows], np.full(len(atom_rows), radius, dtype=np.float32), off, numSD)
        return self._rows(*lead, *columns)

    # ---- radial profiles (no reference counterpart) ---------------------------------------------
    def _radialProfileColumns(self, cols, pick, maxRadius, nShells, numSD):
        """The shells of the atoms ``pick`` of the structure columns over the 2Fo-Fc map at mean + numSD * std (ONE device call), and what
        the parameter tables say about the atoms: (profile dict, atom type per atom -- None without one --, electrons per atom -- NaN without)."""
        _requireParams()
        dm = self.densityObj
        prof = dm.radialProfiles(cols.coord[pick], maxRadius, nShells, dm.meanDensity + numSD * dm.stdDensity)
        tables = _pairTables(cols.pair_names, max(len(cols.pair_names), 1))
        pair = cols.pair_of_atom[pick]
        atom_type = [tables["pair_type"][k] for k in pair.tolist()]
        return prof, atom_type, tables["electrons"][pair] if len(pair) else np.zeros(0)

    def calculateAtomRadialProfiles(self, maxRadius=2.0, nShells=20, numSD=1.5, type=""):
        """One row per atom (``atomRadialProfileHeader``; the atoms and leading columns of ``calculateAtomRegionDensity``): the sphere of
        ``maxRadius`` around the atom cut into ``nShells`` concentric shells of equal width, over the 2Fo-Fc map, in ONE device call
        (``pdbeda_radial_profiles`` in include/pdbeda.h has the contract).  shell_voxels / shell_density: the voxels of a shell and their
        density; shell_significant_*: those above mean + numSD * std (strict) -- each a list of nShells values, innermost shell first.
        atom_type and electrons are None for an atom whose full name the parameter tables do not type.
        A profile is per atom, NOT a partition of the map: bonded atoms share voxels once maxRadius exceeds half a bond length, and
        a shared voxel counts in the profile of each."""
        cols, pick, lead = self._atomPick(type)
        prof, atom_type, electrons = self._radialProfileColumns(cols, pick, maxRadius, nShells, numSD)
        electrons = [None if (t is None or e != e) else e for t, e in zip(atom_type, electrons.tolist())]
        return self._rows(*lead, atom_type, electrons, cols.bfactor[pick], prof["valid"].astype(bool), prof["n"].tolist(), prof["sum"].tolist(),
                          prof["nSig"].tolist(), prof["sumSig"].tolist())

    def atomTypeRadialProfiles(self, maxRadius=2.0, nShells=20, numSD=1.5):
        """One row per atom type present (``atomTypeRadialProfileHeader``), types in sorted order: over the type's atoms that aggregateCloud
        takes (typed, occupancy != 0, in residues with id[0] == ' ') the median, shell by shell, of the cumulative significant density
        around the atom per electron -- the curve the type's radius is read from -- beside ``optimized_radius`` (the parameter tables')
        and ``profile_radius``: the smallest shell outer radius ((k + 1) * maxRadius / nShells) at which that median reaches
        ``densityElectronRatio`` (RuntimeError without a ratio), None when it never does.
        The profiles are per atom, NOT a partition of the map: bonded atoms share voxels once maxRadius exceeds half a bond length, so
        the curve keeps growing past an atom's own density."""
        ratio = self._needRatio()
        cols = _structure.columns(self.biopdbObj)
        tables = _pairTables(cols.pair_names, max(len(cols.pair_names), 1))
        n_atoms = len(cols.atoms)
        eligible = (~cols.res_het)[cols.res_of_atom] & tables["known"][cols.pair_of_atom] & (cols.occupancy != 0) if n_atoms else np.zeros(0, dtype=bool)
        pick = np.nonzero(eligible)[0]
        prof, atom_type, electrons = self._radialProfileColumns(cols, pick, maxRadius, nShells, numSD)
        if len(pick) and np.isnan(electrons).any():      # (aggregateCloud's electronsMap[name] raises the same KeyError)
            raise KeyError(cols.pair_names[int(cols.pair_of_atom[pick][np.isnan(electrons)][0])])
        width = float(np.float32(maxRadius)) / float(nShells)
        outer = [(k + 1) * width for k in range(nShells)]
        per_electron = np.cumsum(prof["sumSig"], axis=1) / electrons[:, None] if len(pick) else np.zeros((0, nShells))
        types = np.asarray(atom_type, dtype=object)
        table = []
        for t in sorted(set(atom_type)):
            rows = np.nonzero(types == t)[0]
            median = np.median(per_electron[rows], axis=0)
            reached = np.nonzero(median >= ratio)[0]
            table.append([t, len(rows), radiiGlobal.get(t), list(outer), median.tolist(), outer[int(reached[0])] if len(reached) else None])
        return table

    # ---- nearest-atom partition of the Fo-Fc map (no reference counterpart) ----------------------
    def _partition(self, maxDistance, numSD):
        """The partition of the Fo-Fc map among ALL symmetry atoms at mean + numSD * std (``pdbeda_map_partition`` in include/pdbeda.h
        has the contract), with the owner volume: computed once per (maxDistance, numSD) and kept, like the blob lists."""
        key = (float(np.float32(maxDistance)), float(numSD))
        if key not in self._partitions:
            coords = self.symmetryAtomCoords
            if len(coords) == 0:
                raise ValueError("XB must be a 2-dimensional array.")       # (the blob table's failure for a file without operators)
            dm = self.diffDensityObj
            self._partitions[key] = dm.partition(np.asarray(coords, dtype=np.float64), maxDistance, dm.meanDensity + numSD * dm.stdDensity, owners=True)
        return self._partitions[key]

    def _partitionColumns(self, atom_rows, maxDistance, numSD):
        """(num_voxels, pos, neg) of the structure's atoms ``atom_rows`` as themselves (the identity images of the symmetry list); an atom
        the list does not hold -- it lies outside the map's box -- owns nothing."""
        ratio = self._needRatio()
        part = self._partition(maxDistance, numSD)
        symmetryAtoms = self.symmetryAtoms
        cols = _structure.columns(self.biopdbObj)
        listed = np.full(len(cols.atoms), -1, dtype=np.int64)
        own = np.nonzero(symmetryAtoms._ident)[0]
        listed[symmetryAtoms._idx[own]] = own
        where = listed[atom_rows]
        have = where >= 0
        pick = lambda column: np.where(have, column[np.where(have, where, 0)], 0).astype(column.dtype) if len(column) else np.zeros(len(where), dtype=column.dtype)
        return ratio, pick(part["n"]), pick(part["sumPos"]), pick(part["sumNeg"])

    @staticmethod
    def _partitionTableColumns(ratio, n, pos, neg):
        absd, net = pos - neg, pos + neg
        return [n, pos, pos / ratio, neg, neg / ratio, absd, absd / ratio, net, net / ratio]

    def calculateAtomPartitionDiscrepancies(self, maxDistance=3.5, numSD=3.0, type=""):
        """One row per atom (``atomPartitionHeader``; the atoms and leading columns of ``calculateAtomRegionDiscrepancies``): the voxels of
        the Fo-Fc map that are nearer to this atom than to any other atom or symmetry image, within ``maxDistance``, and their density
        beyond mean +- numSD * std.  Every voxel is counted for ONE atom, so the rows add up."""
        cols, pick, lead = self._atomPick(type)
        ratio, n, pos, neg = self._partitionColumns(pick, maxDistance, numSD)
        return self._rows(*lead, *self._partitionTableColumns(ratio, n, pos, neg))

    def calculateResiduePartitionDiscrepancies(self, maxDistance=3.5, numSD=3.0, type=""):
        """One row per residue (``residuePartitionHeader``; the leading columns of ``calculateResidueRegionDiscrepancies``): its atoms' rows
        of ``calculateAtomPartitionDiscrepancies`` summed."""
        cols, lead, atom_rows, off = self._residuePick(type, None, False)
        ratio, n, pos, neg = self._partitionColumns(atom_rows, maxDistance, numSD)
        n, pos, neg = _partitionRollup([n, pos, neg], off)
        return self._rows(*lead, *self._partitionTableColumns(ratio, n, pos, neg))

    def partitionSummary(self, maxDistance=3.5, numSD=3.0):
        """The Fo-Fc map's box in three classes -- voxels owned by atoms of the asymmetric unit, by symmetry images, by nobody (farther
        than ``maxDistance`` from every atom: solvent) -- with the noise level where there is no model beside the whole map's."""
        ratio = self._needRatio()
        part = self._partition(maxDistance, numSD)
        dm = self.diffDensityObj
        own = np.asarray(self.symmetryAtoms._ident, dtype=bool)
        box = int(np.prod(part["owner"].shape))
        n_un = int(part["unownedN"][0])
        total, total_pos, total_neg, total_sq = part["unownedSum"].tolist()
        mean = total / n_un if n_un else float("nan")
        std = math.sqrt(max(total_sq / n_un - mean * mean, 0.0)) if n_un else float("nan")
        out = {"max_distance": float(np.float32(maxDistance)), "num_sd": float(numSD), "box_voxels": box,
               "asymmetric_unit_voxels": int(part["n"][own].sum()), "symmetry_voxels": int(part["n"][~own].sum()), "unowned_voxels": n_un,
               "unowned_fraction": n_un / box, "unowned_mean": mean, "unowned_std": std, "map_mean": dm.meanDensity, "map_std": dm.stdDensity}
        for name, pos, neg in (("asymmetric_unit", math.fsum(part["sumPos"][own].tolist()), math.fsum(part["sumNeg"][own].tolist())),
                               ("symmetry", math.fsum(part["sumPos"][~own].tolist()), math.fsum(part["sumNeg"][~own].tolist())), ("unowned", total_pos, total_neg)):
            out[name + "_positive_discrepancy"], out[name + "_negative_discrepancy"] = pos, neg
            out["num_electrons_" + name + "_positive_discrepancy"], out["num_electrons_" + name + "_negative_discrepancy"] = pos / ratio, neg / ratio
        return out

    def _partitionOwners(self, maxDistance):
        """The owner volume at ``maxDistance``: it does not depend on the cutoff, so any partition kept for that distance serves (one at
        numSD 3.0 is made when there is none)."""
        distance = float(np.float32(maxDistance))
        for (d, _), part in self._partitions.items():
            if d == distance:
                return part["owner"]
        return self._partition(maxDistance, 3.0)["owner"]

    def calculateBlobOwnership(self, blobList, maxDistance=3.5):
        """One row per blob of a whole-map list of the Fo-Fc map (``blobOwnershipHeader``): how many of its voxels nobody owns
        (unmodelled density), how many atoms share the rest, and the atom that owns most of them (ties: the lowest symmetry-atom
        index; None columns when nobody owns a voxel).  Host glue over the partition's owner volume."""
        self._needRatio()
        owner = self._partitionOwners(maxDistance)
        if not blobList:
            return []
        if isinstance(blobList, ccp4.DeviceBlobs):
            crs, off = blobList.voxelLists()
        else:
            lists = [sorted(blob.crsList) for blob in blobList]
            crs = np.array([v for one in lists for v in one], dtype=np.int64).reshape(-1, 3)
            off = np.concatenate([[0], np.cumsum([len(one) for one in lists])]).astype(np.int64)
        sizes, unowned, n_owners, main, main_voxels = _blobOwners(owner, crs, off)
        held = np.nonzero(main >= 0)[0]
        atom_rows, symmetry, _ = self.symmetryAtoms.columns(main[held])
        cols = _structure.columns(self.biopdbObj)
        names = {"chain": cols.atom_lists("chain"), "number": cols.atom_lists("number"), "resname": cols.atom_lists("resname"), "name": list(cols.name)}
        columns = {k: [None] * len(sizes) for k in ("chain", "number", "resname", "name", "symmetry")}
        for k, row, sym in zip(held.tolist(), atom_rows.tolist(), symmetry.tolist()):
            for which in names:
                columns[which][k] = names[which][row]
            columns["symmetry"][k] = tuple(sym)
        return [list(row) for row in zip(sizes.tolist(), unowned.tolist(), n_owners.tolist(), columns["chain"], columns["number"], columns["resname"], columns["name"],
                                         columns["symmetry"], main_voxels.tolist())]

    # ---- atom Q-scores over the 2Fo-Fc map (no reference counterpart) -----------------------------
    def _atomQScores(self):
        """(q, n_points, valid) per atom of the structure, from ONE device call kept on the object (``pdbeda_atom_qscores`` in
        include/pdbeda.h has the contract; ``DensityMatrix.qScores`` has the defaults): ALL symmetry atoms compete for the sample
        points, the identity images are scored.  An atom the symmetry list does not hold -- it lies outside the map's box -- has no
        score: NaN, 0 points, not valid."""
        if self._qScores is None:
            coords = self.symmetryAtomCoords
            if len(coords) == 0:
                raise ValueError("XB must be a 2-dimensional array.")       # (the blob table's failure for a file without operators)
            symmetryAtoms = self.symmetryAtoms
            own = np.nonzero(symmetryAtoms._ident)[0]
            got = self.densityObj.qScores(np.asarray(coords, dtype=np.float64), scored=own.astype(np.int32))
            n_atoms = len(_structure.columns(self.biopdbObj).atoms)
            q, n_points, valid = np.full(n_atoms, np.nan), np.zeros(n_atoms, dtype=np.int64), np.zeros(n_atoms, dtype=bool)
            where = symmetryAtoms._idx[own]
            q[where], n_points[where], valid[where] = got["q"], got["nPoints"], got["valid"]
            self._qScores = (q, n_points, valid, got["counters"])
        return self._qScores[:3]

    def calculateAtomQScores(self, type=""):
        """One row per atom (``atomQScoreHeader``; the atoms and leading columns of ``calculateAtomRegionDensity``): the Q-score of the
        atom over the 2Fo-Fc map -- how well the density around it follows a Gaussian, sampled only where this atom is the nearest of
        all symmetry atoms -- with the number of sample points behind it; q_score is None where it is undefined (a flat or non-finite
        neighbourhood, fewer than two shells with a point, an atom outside the map's box)."""
        cols, pick, lead = self._atomPick(type)
        q, n_points, valid = self._atomQScores()
        return self._rows(*lead, cols.bfactor[pick], valid[pick], [None if v != v else v for v in q[pick].tolist()], n_points[pick])

    def calculateResidueQScores(self, type=""):
        """One row per residue (``residueQScoreHeader``; the leading columns of ``calculateResidueRegionDiscrepancies``): the mean and the
        minimum of its atoms' Q-scores over the atoms that have one, and how many those are (None, None, 0 when none has)."""
        cols, lead, atom_rows, off = self._residuePick(type, None, False)
        q = self._atomQScores()[0][atom_rows]
        mean, low, count = [], [], []
        for k in range(len(off) - 1):
            mine = q[off[k]:off[k + 1]]
            mine = mine[~np.isnan(mine)]
            count.append(len(mine))
            mean.append(float(mine.mean()) if len(mine) else None)
            low.append(float(mine.min()) if len(mine) else None)
        return self._rows(*lead, mean, low, count)

    def qScoreSummary(self):
        """Mean and median Q-score, each with the number of atoms behind it, over all atoms that have a score, the backbone (N, CA, C, O
        of residues with id[0] == ' '), the side chains (their other atoms) and the waters (HOH / WAT / DOD): a dict
        ``<class>_mean_q_score`` / ``<class>_median_q_score`` / ``<class>_num_atoms`` (None, None, 0 for an empty class)."""
        cols = _structure.columns(self.biopdbObj)
        q = self._atomQScores()[0]
        names = np.asarray(cols.name, dtype=object)
        het = cols.res_het[cols.res_of_atom] if len(cols.atoms) else np.zeros(0, dtype=bool)
        backbone = np.isin(names, ("N", "CA", "C", "O")) & ~het if len(cols.atoms) else np.zeros(0, dtype=bool)
        water = np.isin(np.asarray(cols.atom_lists("resname"), dtype=object), ("HOH", "WAT", "DOD")) if len(cols.atoms) else np.zeros(0, dtype=bool)
        have = ~np.isnan(q)
        out = {}
        for name, mask in (("all", have), ("backbone", have & backbone), ("side_chain", have & ~het & ~backbone), ("water", have & water)):
            mine = q[mask]
            out[name + "_mean_q_score"] = float(mine.mean()) if len(mine) else None
            out[name + "_median_q_score"] = float(np.median(mine)) if len(mine) else None
            out[name + "_num_atoms"] = int(len(mine))
        return out

    # ---- the calculated density of the model and its agreement with the 2Fo-Fc map (no reference counterpart) ----
    def _modelAtoms(self):
        """What ``modelDensityObj`` is made from: (xyz, amp, expo, radii, electrons placed) of ALL symmetry atoms whose 'RES_ATOM' name has
        electrons in the parameter tables and whose occupancy is not 0 (the atoms ``aggregateCloud`` would not skip), under the
        single-Gaussian model of ``ccp4.gaussianAtomTerms`` with the module's ``modelBlur`` and ``modelSigmas``."""
        _requireParams()
        coords = np.asarray(self.symmetryAtomCoords, dtype=np.float64).reshape(-1, 3)
        cols = _structure.columns(self.biopdbObj)
        rows = self.symmetryAtoms._idx
        names = cols.pair_names
        electrons = _pairTables(names, max(len(names), 1))["electrons"][cols.pair_of_atom[rows]] if len(rows) else np.zeros(0)
        occupancy = cols.occupancy[rows] if len(rows) else np.zeros(0)
        keep = ~np.isnan(electrons) & (occupancy != 0)
        amp, expo, bEff = ccp4.gaussianAtomTerms(electrons[keep], cols.bfactor[rows][keep] if len(rows) else np.zeros(0), occupancy[keep], blur=modelBlur)
        return coords[keep], amp, expo, ccp4.modelRadii(bEff, modelSigmas), float(np.sum(electrons[keep] * occupancy[keep]))

    @property
    def modelDensityObj(self):
        """The calculated density of the model on the grid of the 2Fo-Fc map, in electrons per A^3, made on the device on first use
        (``DensityMatrix.modelDensity``).  It never leaves HBM unless somebody reads ``.density``."""
        if self._model is None:
            xyz, amp, expo, radii, placed = self._modelAtoms()
            self._model = (self.densityObj.modelDensity(xyz, amp, expo, radii), placed)
        return self._model[0]

    def modelCorrelation(self, floor=None):
        """``densityObj.correlate(modelDensityObj, floor)``: n, cc, and the scale and offset of 2Fo-Fc ~ scale * model + offset over the
        voxels of the non-repeating box (with ``floor``: only where the model exceeds it -- the part of the map the model says is
        occupied)."""
        return self.densityObj.correlate(self.modelDensityObj, floor)

    @property
    def modelDifferenceObj(self):
        """2Fo-Fc - scale * model on the device (``pdbeda_map_combine``), scale from ``modelCorrelation()``: an observed-minus-model map that
        ``createFullBlobList`` / ``findPeaks`` and everything behind them take as it is.  Leave a ligand out of the structure and this
        is its omit map."""
        if self._modelDifference is None:
            d, model = self.densityObj, self.modelDensityObj
            scale = self.modelCorrelation()["scale"]
            if scale != scale:
                raise RuntimeError("the model density is constant over the map: there is no scale to subtract it with")
            self._modelDifference = ccp4.DensityMatrix.fromDeviceMap(d.header, d.origin, type(d._map).combine(d._map, model._map, -scale), d.pdbid, d._ctx)
        return self._modelDifference

    def _modelRsccRsr(self, groups, radius):
        """``_rsccRsr`` against the calculated map: the model's density at the gathered voxels, brought to the observed map's scale by the
        whole-map fit of ``modelCorrelation()`` (RSR compares magnitudes; RSCC does not see the fit)."""
        fit = self.modelCorrelation()
        model = self.modelDensityObj._map
        return self._groupCorrelations(groups, radius, lambda crs, fo: model.point_density(crs) * fit["scale"] + fit["offset"])

    def calculateAtomModelCorrelations(self, radius=None):
        """One row per atom (``atomModelCorrelationHeader``; the atoms and leading columns of ``calculateAtomRegionDensity``): RSCC and RSR
        of the 2Fo-Fc map against the calculated map over the sphere of ``radius`` around the atom (None: the resolution-dependent
        radius of ``atomMetrics``) -- ``atomMetrics`` with a calculated map that comes from the atoms instead of from the two observed
        maps.  None where a value is undefined."""
        cols, pick, lead = self._atomPick("")
        radius = self._metricsRadius() if radius is None else radius
        rscc, rsr = self._modelRsccRsr([[c] for c in cols.coord[pick]], radius)
        clean = lambda v: [None if x != x else x for x in v.tolist()]
        return self._rows(*lead, cols.bfactor[pick], clean(rscc), clean(rsr))

    def calculateResidueModelCorrelations(self, radius=None):
        """One row per residue (``residueModelCorrelationHeader``; the leading columns of ``calculateResidueRegionDiscrepancies``): RSCC and
        RSR of the 2Fo-Fc map against the calculated map over the de-duplicated union of the spheres of its atoms."""
        cols, lead, atom_rows, off = self._residuePick("", None, False)
        radius = self._metricsRadius() if radius is None else radius
        coord = cols.coord[atom_rows]
        rscc, rsr = self._modelRsccRsr([coord[off[k]:off[k + 1]] for k in range(len(off) - 1)], radius)
        clean = lambda v: [None if x != x else x for x in v.tolist()]
        return self._rows(*lead, clean(rscc), clean(rsr))

    def modelSummary(self):
        """The whole-map agreement of the model: ``cc``, ``scale``, ``offset`` and ``n`` of ``modelCorrelation()``, ``electrons_placed`` (sum
        of occupancy * Z over the symmetry atoms the map was made from) and ``electrons_found`` (sum of the calculated map over the
        non-repeating box times the voxel volume: the electrons that landed inside the box, less what the cut-off radius drops)."""
        model = self.modelDensityObj
        fit = self.modelCorrelation()
        total = model.pairMoments(model)[1]
        return {"cc": fit["cc"], "scale": fit["scale"], "offset": fit["offset"], "n": fit["n"], "electrons_placed": self._model[1],
                "electrons_found": total * self.densityObj.header.unitVolume}

    # ---- the way back from the maps to the atoms: gradients of the map-model target, real-space refinement (no reference counterpart) ----
    def _refinementAtoms(self):
        """What the gradient and refinement calls work on: a dict ``atomRows`` (rows of the structure columns of the atoms of the asymmetric
        unit that ``modelDensityObj`` places: electrons known, occupancy not 0), their ``xyz``, ``electrons``, ``bfactors`` and
        ``occupancies``, and for every symmetry atom the model is made from -- in ``_modelAtoms``' order -- ``rows`` (its atom, as an index
        into ``atomRows``) and ``operators`` ([R | t] with the lattice translation of its cell folded into t; the operator index is the
        fourth entry of the symmetry tag that ``symmetryAtoms.columns`` gives)."""
        _requireParams()
        cols = _structure.columns(self.biopdbObj)
        names = cols.pair_names
        n = len(cols.atoms)
        electrons = _pairTables(names, max(len(names), 1))["electrons"][cols.pair_of_atom] if n else np.zeros(0)
        occupancy = np.asarray(cols.occupancy, dtype=np.float64) if n else np.zeros(0)
        keep = ~np.isnan(electrons) & (occupancy != 0)
        kept = np.nonzero(keep)[0]
        position = np.full(n, -1, dtype=np.int64)
        position[kept] = np.arange(len(kept))
        sym = self.symmetryAtoms
        idx, tags = np.asarray(sym._idx, dtype=np.int64), np.asarray(sym._sym, dtype=np.int64).reshape(-1, 4)
        use = keep[idx] if len(idx) else np.zeros(0, dtype=bool)
        rot = np.array([np.asarray(m, dtype=np.float64) for m in self.pdbObj.header.rotationMats]).reshape(-1, 3, 4)
        ortho = np.asarray(self.densityObj.header.orthoMat, dtype=np.float64)
        operators = rot[tags[use, 3]].copy() if use.any() else np.zeros((0, 3, 4))
        if len(operators):
            operators[:, :, 3] += tags[use, :3].astype(np.float64).dot(ortho.T)
        return {"atomRows": kept, "xyz": np.asarray(cols.coord, dtype=np.float64).reshape(-1, 3)[kept], "electrons": electrons[kept],
                "bfactors": np.asarray(cols.bfactor, dtype=np.float64)[kept], "occupancies": occupancy[kept], "rows": position[idx[use]], "operators": operators}

    def _atomGradients(self):
        """(atoms of ``_refinementAtoms``, dT/dtheta folded over the images, the Gauss-Newton step, pairs per atom, the fit) at the deposited model."""
        atoms = self._refinementAtoms()
        d, model = self.densityObj, self.modelDensityObj
        target, scale, offset, cc = d._leastSquaresTarget(model)
        xyz, amp, expo, radii, _ = self._modelAtoms()
        rows, n = atoms["rows"], len(atoms["atomRows"])
        got = d._residual(model, scale, offset).atomMoments(xyz, expo, radii, uniqueBox=True)
        each = ccp4.gaussianAtomGradients(got["moments"], atoms["electrons"][rows], atoms["bfactors"][rows], atoms["occupancies"][rows], blur=modelBlur)
        folded = ccp4.foldImageGradients(each, rows, atoms["operators"][:, :, :3], n)
        gradT = {k: -scale * v for k, v in folded.items()}
        copies = np.bincount(rows, minlength=n).astype(np.float64)
        curv = ccp4.gaussianAtomCurvatures(atoms["electrons"], atoms["bfactors"], atoms["occupancies"], d.header.unitVolume, blur=modelBlur)
        step = ccp4.gaussNewtonStep(gradT, {k: v * copies for k, v in curv.items()}, scale, ("xyz", "b", "occ"), refineMaxShift)
        pairs = np.zeros(n, dtype=np.int64)
        np.add.at(pairs, rows, got["nVoxels"].astype(np.int64))
        return atoms, gradT, step, pairs, {"T": target, "scale": scale, "offset": offset, "cc": cc}

    def calculateAtomGradients(self):
        """One row per atom of the asymmetric unit (``atomGradientHeader``; the atoms and leading columns of
        ``calculateAtomRegionDensity``): the derivatives of T = sum (2Fo-Fc - s model - o)^2 / 2 over the non-repeating box -- s and o the
        fit of ``modelCorrelation()`` -- with respect to the atom's x, y, z, B and occupancy, the damped Gauss-Newton shift each implies
        (``ccp4.gaussNewtonStep``; the position shift capped at the module's ``refineMaxShift``) and the voxel pairs the sums ran over.
        The contributions of the atom's symmetry copies are folded in: a copy's positional gradient comes back through the transpose
        of its operator's rotation.  An atom the model does not place (no electrons known, occupancy 0) has zeros: T does not depend
        on it."""
        cols, pick, lead = self._atomPick("")
        atoms, gradT, step, pairs, _ = self._atomGradients()
        n, at = len(cols.atoms), atoms["atomRows"]
        table = np.zeros((n, 10))
        table[at, 0:3], table[at, 3], table[at, 4] = gradT["dXyz"], gradT["dB"], gradT["dOcc"]
        table[at, 5:8], table[at, 8], table[at, 9] = step["xyz"], step["b"], step["occ"]
        count = np.zeros(n, dtype=np.int64)
        count[at] = pairs
        return self._rows(*lead, cols.bfactor[pick], *[table[:, k] for k in range(10)], count)

    def refineAtoms(self, what=("xyz", "b"), cycles=None):
        """Real-space refinement of the deposited atoms against the 2Fo-Fc map (``DensityMatrix.refineGaussianAtoms`` on the atoms of the
        asymmetric unit, their symmetry copies following them): one row per atom (``refineAtomHeader``) with the refined coordinate, B
        and occupancy, the length of the shift and the change of B.  The structure itself is left as it is; the result of the last call
        is kept for ``refineSummary``.  ``cycles`` defaults to the module's ``refineCycles``."""
        cols, pick, lead = self._atomPick("")
        atoms = self._refinementAtoms()
        out = self.densityObj.refineGaussianAtoms(atoms["xyz"], atoms["electrons"], atoms["bfactors"], atoms["occupancies"], what=tuple(what),
                                                  cycles=refineCycles if cycles is None else cycles, maxShift=refineMaxShift,
                                                  imageAtoms=(atoms["rows"], atoms["operators"]), blur=modelBlur, nSigma=modelSigmas)
        self._refined = (atoms, out)
        n, at = len(cols.atoms), atoms["atomRows"]
        xyz = np.asarray(cols.coord, dtype=np.float64).reshape(-1, 3).copy()
        b, occ = np.asarray(cols.bfactor, dtype=np.float64).copy(), np.asarray(cols.occupancy, dtype=np.float64).copy()
        xyz[at], b[at], occ[at] = out["xyz"], out["bfactors"], out["occupancies"]
        shift, deltaB = np.zeros(n), np.zeros(n)
        shift[at] = np.sqrt(((out["xyz"] - atoms["xyz"]) ** 2).sum(axis=1))
        deltaB[at] = out["bfactors"] - atoms["bfactors"]
        return self._rows(*lead, cols.bfactor[pick], xyz[:, 0], xyz[:, 1], xyz[:, 2], b, occ, shift, deltaB)

    def refineSummary(self):
        """T, the correlation and the scale before and after the last ``refineAtoms`` call (made with its defaults when there was none), the
        cycles run, and the rms shift and rms change of B over the refined atoms."""
        if self._refined is None:
            self.refineAtoms()
        atoms, out = self._refined
        trace = out["trace"]
        n = max(len(atoms["atomRows"]), 1)
        return {"num_atoms": len(atoms["atomRows"]), "cycles": len(trace["halvings"]), "target_before": trace["T"][0], "target_after": trace["T"][-1],
                "cc_before": trace["cc"][0], "cc_after": trace["cc"][-1], "scale_before": trace["scale"][0], "scale_after": trace["scale"][-1],
                "rms_shift": float(np.sqrt(((out["xyz"] - atoms["xyz"]) ** 2).sum() / n)), "rms_delta_b": float(np.sqrt(((out["bfactors"] - atoms["bfactors"]) ** 2).sum() / n))}

    # ---- what fits in a green blob: rigid-fragment pose search on the Fo-Fc map (no reference counterpart) ----
    def _fitScoreMap(self, penalty):
        """The map a fragment is scored on: Fo-Fc - penalty * ``atomMask`` of ALL symmetry atoms (van der Waals spheres, ``ccp4.maskRadii`` by
        element), made by the existing ``atomMask`` and ``pdbeda_map_combine`` calls as a resident map, kept per penalty."""
        key = ("fitScore", float(penalty))
        if key not in self._local:
            diff = self.diffDensityObj
            if penalty == 0.0:
                self._local[key] = diff
            else:
                cols = _structure.columns(self.biopdbObj)
                rows = np.asarray(self.symmetryAtoms._idx, dtype=np.int64)
                coords = np.asarray(self.symmetryAtomCoords, dtype=np.float64).reshape(-1, 3)
                elements = [getattr(cols.atoms[r], "element", "") or "" for r in rows]
                mask = diff.atomMask(coords, ccp4.maskRadii(elements) if len(rows) else np.zeros(0))
                self._local[key] = ccp4.DensityMatrix.fromDeviceMap(diff.header, diff.origin, type(diff._map).combine(diff._map, mask._map, -float(penalty)), diff.pdbid, diff._ctx)
        return self._local[key]

    def _blobCentres(self, blob):
        """The voxel centres of a blob, thinned evenly to ``fitMaxCentres``."""
        crs = np.asarray(sorted(blob.crsList), dtype=np.int64).reshape(-1, 3)
        if len(crs) > fitMaxCentres:
            crs = crs[np.linspace(0, len(crs) - 1, fitMaxCentres).astype(np.int64)]
        return np.asarray(self.diffDensityObj.header.crs2xyz_array(crs), dtype=np.float64).reshape(-1, 3)

    def fitFragment(self, fragment, blob=None, centres=None, nRotations=None, topK=5, penalty=None, refine=True):
        """Where a rigid ``fragment`` (``fragmentFromResidue``, or a dict ``xyz`` / ``electrons``) sits best in unexplained density: every pose
        (centre, rotation) is scored on the device (``DensityMatrix.searchFragment`` / ``pdbeda_pose_scores``) by sum_a electrons_a * rho(atom a) on
        the SCORE MAP, Fo-Fc minus ``penalty`` times the ``atomMask`` of the symmetry atoms.  Clash avoidance therefore costs no kernel code; the
        interpolation smears the mask's edge over one voxel, so it is a SOFT penalty: an atom half a voxel inside a neighbour's sphere pays about
        half of it.  ``centres`` default to the voxel centres of ``blob`` (a green blob or its index in ``greenBlobList``; None: the largest), or
        pass the blob's peaks.  ``penalty`` defaults to ``fitPenaltyCutoffs`` Fo-Fc cut-offs.  The lattice pass scores ``nRotations``
        (``fitRotations``) rotations at every centre; with ``refine`` the ``topK`` best poses are polished coarse to fine, every level one device
        call.  Returns ``topK`` rows at the most, best first (``blobFitHeader`` without its two leading blob columns): rank, centre, rotation (9
        numbers, row-major), score, the atoms that read below 0 on the score map, the RSCC of the placed fragment -- its ``modelDensity`` (B 20,
        the module's blur) against the Fo-Fc map where the model exceeds 0 (``correlate``) --, and the placed coordinates."""
        frame = ccp4.fragmentFrame(fragment["xyz"], fragment.get("electrons"))
        if centres is None:
            blobs = self.greenBlobList
            if blob is None:
                if not len(blobs):
                    return []
                blob = max(range(len(blobs)), key=lambda i: blobs[i].numVoxels)
            centres = self._blobCentres(blobs[blob] if isinstance(blob, (int, np.integer)) else blob)
        centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        if not len(centres) or not len(frame["xyz"]):
            return []
        diff = self.diffDensityObj
        cutoff = float(diff.diffDensityCutoff)
        score = self._fitScoreMap(fitPenaltyCutoffs * cutoff if penalty is None else float(penalty))
        n_rot = int(fitRotations if nRotations is None else nRotations)
        poses = score.searchFragment(frame["xyz"], frame["weights"], centres, nRotations=n_rot, nBest=int(topK), levels=4 if refine else 0, floor=0.0, allowOutside=True)
        rows = []
        z = np.asarray(frame["weights"], dtype=np.float64)
        amp, expo, bEff = ccp4.gaussianAtomTerms(z, np.full(len(z), 20.0), np.ones(len(z)), blur=modelBlur)
        radii = ccp4.modelRadii(bEff, modelSigmas)
        for rank, pose in enumerate(poses):
            fit = diff.correlate(diff.modelDensity(pose["xyz"], amp, expo, radii), floor=0.0)
            rscc = None if fit["cc"] != fit["cc"] else float(fit["cc"])
            rows.append([rank, [float(v) for v in pose["centre"]], [float(v) for v in pose["rotation"].reshape(-1)], float(pose["score"]), int(pose["low"]), rscc,
                         [[float(v) for v in p] for p in pose["xyz"]]])
        return rows

    def calculateBlobFits(self, fragment, minElectrons=None, topK=1, **kw):
        """``fitFragment`` over every green blob large enough to hold the fragment: one row per blob and rank (``blobFitHeader``).  A blob
        is large enough when its volume is at least ``fitMinVolumePerAtom`` (half a cubic Angstrom: the core a 3 sigma contour leaves of an atom
        is a few times that; specks of noise are far below it) times the fragment's atoms, or, with ``minElectrons``, when its density
        integrates to that many electrons (``densityElectronRatio``, which needs the atom clouds)."""
        blobs = self.greenBlobList
        n_atoms = len(np.asarray(fragment["xyz"]).reshape(-1, 3))
        voxel = float(self.diffDensityObj.header.unitVolume)
        out = []
        for i in range(len(blobs)):
            blob = blobs[i]
            if minElectrons is None:
                enough = blob.numVoxels * voxel >= n_atoms * fitMinVolumePerAtom
            else:
                if not self.densityElectronRatio:
                    raise RuntimeError("Failed to calculate densityElectronRatio, probably due to total aggregated electrons less than the minimum.")
                enough = abs(blob.totalDensity / self.densityElectronRatio) >= float(minElectrons)
            if enough:
                out += [[i, int(blob.numVoxels)] + row for row in self.fitFragment(fragment, blob=i, topK=topK, **kw)]
        return out

    def defaultFitFragment(self, resname=""):
        """The fragment of the "fit" mode: the first residue of the structure called ``resname``; by default the first hetero residue that is
        not water, else the first residue."""
        residues = list(self.biopdbObj.get_residues())
        if resname:
            named = [r for r in residues if r.resname.strip() == resname.strip()]
        else:
            named = [r for r in residues if r.id[0].strip() not in ("", "W")] or residues
        if not named:
            raise ValueError("no residue %r in the structure to take the fragment from" % resname)
        return fragmentFromResidue(named[0])

    # ---- local statistics: significance against the surroundings, local map-model correlation (no reference counterpart) ----
    def _localTaps(self, densityObj):
        """The Gaussian window of ``localWindowSigma`` A, cut off at ``localWindowTruncate`` standard deviations, as taps per crs axis: the
        sigma in grid steps of an axis is sigma / gridLength of the cell axis it runs along.  On an orthogonal cell this is
        ``DensityMatrix.gaussianFilter``'s window; on a skewed cell the window is a Gaussian along the cell axes, which is what a separable
        filter can do there."""
        header = densityObj.header
        taps = [ccp4.gaussianTaps(localWindowSigma / header.gridLength[header.map2crs[k]], localWindowTruncate) for k in range(3)]
        for axis, t in zip("crs", taps):
            if len(t) // 2 > ccp4.FILTER_MAX_RADIUS:
                raise ValueError("the local window reaches radius %d along %s, beyond the filter's largest radius %d" % (len(t) // 2, axis, ccp4.FILTER_MAX_RADIUS))
        return taps

    @property
    def localDiffStats(self):
        """``diffDensityObj.localStats`` under the module's window: ``mean``, ``std`` and ``z`` of the Fo-Fc map as device-made maps, the
        local standard deviation never taken below ``localStdFloorFraction`` of the map's own."""
        if "diff" not in self._local:
            diff = self.diffDensityObj
            self._local["diff"] = diff.localStats(taps=self._localTaps(diff), stdFloor=localStdFloorFraction * diff.stdDensity)
        return self._local["diff"]

    @property
    def localZDiffObj(self):
        """The Fo-Fc map in local standard deviations from its local mean: what a blob search cuts at +-3 to find density that is
        significant against ITS surroundings, bulk solvent or protein core."""
        return self.localDiffStats["z"]

    def _localGreenRed(self):
        if "blobs" not in self._local:
            self._local["blobs"] = self.localZDiffObj.createFullBlobLists(3.0)
        return self._local["blobs"]

    @property
    def localGreenBlobList(self):
        """``createFullBlobList(3)`` on ``localZDiffObj``: the green blobs that stand out of their surroundings (totalDensity is in z units)."""
        return self._localGreenRed()[0]

    @property
    def localRedBlobList(self):
        """``createFullBlobList(-3)`` on ``localZDiffObj``."""
        return self._localGreenRed()[1]

    @property
    def localModelCorrelationObj(self):
        """The correlation of the 2Fo-Fc map with ``modelDensityObj`` inside the window around every voxel, as a device-made map in
        [-1, 1] (0 where either map is locally flat): where on the grid the model explains the density, which the one number of
        ``modelCorrelation()`` cannot say."""
        if "cc" not in self._local:
            dens = self.densityObj
            made = dens._map.local_stats(self.modelDensityObj._map, *self._localTaps(dens), std_floor=0.0, want=("cc",))
            self._local["cc"] = dens._made(made["cc"])
        return self._local["cc"]

    def _atomLocalValues(self, coord):
        """(local_cc, local_z_diff, local_std_diff) at the coordinates, read by trilinear interpolation."""
        xyz = np.asarray(coord, dtype=np.float64).reshape(-1, 3)
        if len(xyz) == 0:
            return np.zeros(0), np.zeros(0), np.zeros(0)
        stats = self.localDiffStats
        return (np.asarray(self.localModelCorrelationObj.getInterpolatedDensityFromXyz(xyz), dtype=np.float64),
                np.asarray(stats["z"].getInterpolatedDensityFromXyz(xyz), dtype=np.float64), np.asarray(stats["std"].getInterpolatedDensityFromXyz(xyz), dtype=np.float64))

    def calculateAtomLocalCorrelations(self):
        """One row per atom (``atomLocalHeader``; the atoms and leading columns of ``calculateAtomModelCorrelations``): the local map-model
        correlation, the local z-score of the Fo-Fc map and its local standard deviation, each read at the atom's position with
        ``getInterpolatedDensityFromXyz``."""
        cols, pick, lead = self._atomPick("")
        cc, z, std = self._atomLocalValues(cols.coord[pick])
        return self._rows(*lead, cols.bfactor[pick], cc, z, std)

    def calculateResidueLocalCorrelations(self):
        """One row per residue (``residueLocalHeader``): the mean and the minimum ``local_cc`` of its atoms and the ``local_z_diff`` of largest
        magnitude among them, with its sign (None for a residue without atoms)."""
        cols, lead, atom_rows, off = self._residuePick("", None, False)
        cc, z, _ = self._atomLocalValues(cols.coord[atom_rows])
        mean, low, extreme = [], [], []
        for k in range(len(off) - 1):
            mine, zs = cc[off[k]:off[k + 1]], z[off[k]:off[k + 1]]
            mean.append(float(mine.mean()) if len(mine) else None)
            low.append(float(mine.min()) if len(mine) else None)
            extreme.append(float(zs[int(np.argmax(np.abs(zs)))]) if len(zs) else None)
        return self._rows(*lead, mean, low, extreme)

    def localSummary(self):
        """The window (``window_sigma`` in A, ``window_truncate``, ``radius_c`` / ``radius_r`` / ``radius_s`` in grid steps), the numbers of
        green and red blobs that are significant locally and globally, and the median and minimum ``local_cc`` over the atoms."""
        radii = [len(t) // 2 for t in self._localTaps(self.diffDensityObj)]
        cols, pick, _ = self._atomPick("")
        cc = self._atomLocalValues(cols.coord[pick])[0]
        return {"window_sigma": localWindowSigma, "window_truncate": localWindowTruncate, "radius_c": radii[0], "radius_r": radii[1], "radius_s": radii[2],
                "num_local_green_blobs": len(self.localGreenBlobList), "num_local_red_blobs": len(self.localRedBlobList),
                "num_green_blobs": len(self.greenBlobList), "num_red_blobs": len(self.redBlobList),
                "median_atom_local_cc": float(np.median(cc)) if len(cc) else None, "min_atom_local_cc": float(cc.min()) if len(cc) else None}

    # ---- two entries on one grid, and the whole unit cell: maps resampled under coordinate operators (no reference counterpart) ----
    def operatorTo(self, other, atomName="CA"):
        """(op, rmsd, n): the proper rigid motion that carries THIS entry's coordinates onto ``other``'s -- ``ccp4.kabschOperator`` over the
        atoms named ``atomName`` (all names when empty) that both entries have under the same chain, residue number and atom name -- the
        root-mean-square distance it leaves, and the number of matched atoms.  It is the pull-back that ``compareMaps`` needs: a voxel of
        this entry's grid is carried to the place in ``other`` that holds the same part of the molecule.  Fewer than three matches raise."""
        def keyed(analyzer):
            cols, pick, lead = analyzer._atomPick(atomName)
            found = {}
            for row, chain, number, name in zip(pick.tolist(), lead[1], lead[2], lead[4]):
                found.setdefault((chain, number, name), row)      # (the first of alternate locations)
            return cols, found
        mine, here = keyed(self)
        theirs, there = keyed(other)
        shared = [key for key in here if key in there]
        if len(shared) < 3:
            raise ValueError("operatorTo: %d atoms named %r match by chain, residue number and name; three are needed" % (len(shared), atomName))
        op, rmsd = ccp4.kabschOperator(np.asarray(mine.coord, dtype=np.float64)[[here[k] for k in shared]], np.asarray(theirs.coord, dtype=np.float64)[[there[k] for k in shared]])
        return op, rmsd, len(shared)

    def _operatorFor(self, other, operator):
        if operator is None:
            op, rmsd, _ = self.operatorTo(other)
            return op, rmsd
        return ccp4._operator(operator), None

    def _otherOnMyGrid(self, other, operator, order):
        """``other``'s 2Fo-Fc map on this entry's grid, NaN where it has nothing, with the operator and its rmsd."""
        op, rmsd = self._operatorFor(other, operator)
        return other.densityObj.resampled(self.densityObj.header, op.reshape(1, 12), order=order, fill=float("nan")), op, rmsd

    def compareMaps(self, other, operator=None, order=1):
        """``other``'s 2Fo-Fc map against this entry's, on THIS entry's grid: ``other``'s map is resampled under ``operator`` (this entry's
        coordinates to ``other``'s; default: ``operatorTo(other)``) with a NaN fill and correlated with this one over the voxels it covers
        (``DensityMatrix.correlate`` skips what is not finite).  A dict: ``n``, ``cc``, ``scale`` and ``offset`` of mine ~ scale * other +
        offset, ``coveredFraction`` of this entry's stored voxels, ``rmsd`` of the operator (None for a given one) and ``operator``."""
        moved, op, rmsd = self._otherOnMyGrid(other, operator, order)
        fit = self.densityObj.correlate(moved)
        counters = moved.resampleCounters
        fit.update({"coveredFraction": counters["covered"] / float(counters["covered"] + counters["uncovered"]), "rmsd": rmsd, "operator": op})
        return fit

    def isomorphousDifferenceObj(self, other, operator=None, order=1):
        """This entry's 2Fo-Fc map minus ``scale`` times ``other``'s, on this entry's grid, as a device-made DensityMatrix: ``scale`` from
        ``compareMaps``, the subtraction inside ONE resample call (``base`` = this map, ``alpha`` = -scale); 0 where ``other`` has nothing.
        ``createFullBlobList``, ``findPeaks`` and the basins take it as it is: what one entry has and the other lacks -- a ligand, a
        moved loop."""
        fit = self.compareMaps(other, operator, order)
        if fit["scale"] != fit["scale"]:
            raise RuntimeError("the other entry's map is constant where it covers this one: there is no scale to subtract it with")
        return other.densityObj.resampled(self.densityObj.header, fit["operator"].reshape(1, 12), order=order, fill=0.0, base=self.densityObj, alpha=-fit["scale"])

    def _expanded(self, densityObj, order):
        return densityObj.symmetryExpanded([np.asarray(m, dtype=np.float64) for m in self.pdbObj.header.rotationMats], order=order)

    @property
    def expandedDensityObj(self):
        """The 2Fo-Fc map over the WHOLE unit cell (``DensityMatrix.symmetryExpanded`` with the header's ``rotationMats``): PDBe maps are
        cut-outs around the model, this is the density under every symmetry mate too."""
        if "expanded" not in self._local:
            self._local["expanded"] = self._expanded(self.densityObj, 1)
        return self._local["expanded"]

    @property
    def expandedDiffDensityObj(self):
        """The Fo-Fc map over the whole unit cell."""
        if "expandedDiff" not in self._local:
            self._local["expandedDiff"] = self._expanded(self.diffDensityObj, 1)
        return self._local["expandedDiff"]

    # ---- reciprocal space: the 2Fo-Fc map of the whole cell against the model, shell by shell (no reference counterpart) ----
    def _cellAtoms(self, header):
        """(xyz, amp, expo, radii) of every atom copy whose cut-off sphere reaches the unit cell of ``header``: the model's atoms (those
        ``_modelAtoms`` keeps, taken from the asymmetric unit) under the identity and the distinct operators of the header's
        ``rotationMats``, each brought into the cell by whole lattice translations, and its 26 neighbours where the sphere crosses a face."""
        _requireParams()
        cols = _structure.columns(self.biopdbObj)
        names = cols.pair_names
        electrons = _pairTables(names, max(len(names), 1))["electrons"][cols.pair_of_atom] if len(cols.coord) else np.zeros(0)
        keep = ~np.isnan(electrons) & (cols.occupancy != 0) if len(cols.coord) else np.zeros(0, dtype=bool)
        amp, expo, bEff = ccp4.gaussianAtomTerms(electrons[keep], cols.bfactor[keep], cols.occupancy[keep], blur=modelBlur)
        radii = ccp4.modelRadii(bEff, modelSigmas)
        xyz = np.asarray(cols.coord, dtype=np.float64).reshape(-1, 3)[keep]
        copies, rows = self._cellCopies(header, xyz, float(radii.max()) if len(radii) else 0.0)
        return copies, amp[rows], expo[rows], radii[rows]

    def _cellCopies(self, header, xyz, reach):
        """(xyz of the copies, the row of ``xyz`` each came from): the atoms ``xyz`` under the identity and the distinct operators of the header's
        ``rotationMats``, each brought into the unit cell of ``header`` by whole lattice translations, and its 26 neighbours where a sphere of
        ``reach`` Angstrom around it crosses a face of the cell."""
        ops, seen = [], set()
        for op in [ccp4.identityOperator()] + [ccp4._operator(m) for m in self.pdbObj.header.rotationMats]:
            key = tuple(np.round(op.reshape(-1), 5).tolist())
            if key not in seen:
                seen.add(key)
                ops.append(op)
        ortho, deortho = np.asarray(header.orthoMat, dtype=np.float64), np.asarray(header.deOrthoMat, dtype=np.float64)
        pad = float(reach) * np.sqrt((deortho ** 2).sum(axis=1)) if len(xyz) else np.zeros(3)      # the sphere's reach in fractional units
        shifts = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
        out_xyz, out_row = [], []
        for op in ops:
            frac = ccp4.applyOperator(op, xyz).dot(deortho.T)
            frac -= np.floor(frac)
            for shift in shifts:
                f = frac + shift
                inside = ((f >= -pad) & (f <= 1.0 + pad)).all(axis=1)
                out_xyz.append(f[inside].dot(ortho.T))
                out_row.append(np.nonzero(inside)[0])
        rows = np.concatenate(out_row) if out_row else np.zeros(0, dtype=np.int64)
        return (np.concatenate(out_xyz) if out_xyz else np.zeros((0, 3))), rows

    def _fourierMaps(self):
        """(observed, model): the 2Fo-Fc map over the whole unit cell -- ``expandedDensityObj`` where the cell's sampling can be transformed,
        else the tricubic expansion onto ``ccp4.fourierHeader`` -- and the calculated density of every atom copy of the cell on that grid.
        Both stay in HBM."""
        if "fourier" not in self._local:
            header = self.densityObj.header
            if all(ccp4.isFourierSize(n) for n in header.crsInterval):
                observed = self.expandedDensityObj
            else:
                observed = self.densityObj.symmetryExpanded([np.asarray(m, dtype=np.float64) for m in self.pdbObj.header.rotationMats], header=ccp4.fourierHeader(header), order=3)
            xyz, amp, expo, radii = self._cellAtoms(observed.header)
            self._local["fourier"] = (observed, observed.modelDensity(xyz, amp, expo, radii))
        return self._local["fourier"]

    def modelShellTable(self, nShells=20):
        """The 2Fo-Fc map against the model per resolution shell (``DensitySpectrum.shells`` of the two whole-cell maps of ``_fourierMaps``,
        ``nShells`` shells of equal reciprocal volume up to the grid's Nyquist limit): a dict of arrays ``d_max``, ``d_min``, ``n``,
        ``power``, ``powerOther`` (the model's), ``fsc``, ``phaseCosine`` and ``scale`` (2Fo-Fc ~ scale * model)."""
        key = ("shells", int(nShells))
        if key not in self._local:
            observed, model = self._fourierMaps()
            self._local[key] = observed.shellStats(model, nShells)
        return self._local[key]

    def fscResolution(self, threshold=0.5, nShells=20):
        """The resolution in Angstrom at which the map-model Fourier shell correlation first falls through ``threshold``: the first pair of
        consecutive shells with fsc[j] >= threshold > fsc[j + 1], linearly interpolated in s between the shells' mid points (s = 1 / d).
        None if the curve never crosses."""
        table = self.modelShellTable(nShells)
        s = 0.5 * (1.0 / table["d_max"] + 1.0 / table["d_min"])
        fsc = table["fsc"]
        for j in range(len(fsc) - 1):
            a, b = fsc[j], fsc[j + 1]
            if np.isfinite(a) and np.isfinite(b) and a >= threshold > b:
                return 1.0 / float(s[j] + (a - threshold) / (a - b) * (s[j + 1] - s[j]))
        return None

    def resolutionCutDensityObj(self, d, dMax=None, softness=0.1):
        """The whole-cell 2Fo-Fc map cut at ``d`` Angstrom (``DensityMatrix.resolutionCut``), as a device-made DensityMatrix that the blob and
        peak searches take as it is."""
        return self._fourierMaps()[0].resolutionCut(d, dMax, softness)

    def sharpenedDensityObj(self, B):
        """The whole-cell 2Fo-Fc map with the B-factor ``B`` applied in reciprocal space (negative sharpens)."""
        return self._fourierMaps()[0].sharpened(B)

    def fourierSummary(self, nShells=20):
        """The grid that was transformed (``grid_c`` / ``grid_r`` / ``grid_s``), its Nyquist limit ``d_min``, the resolutions at which the map-model
        FSC falls through 0.5 and 0.143 (None: it does not), the FSC and the scale over all shells together, and the number of shells."""
        table = self.modelShellTable(nShells)
        sums = table["sums"].sum(axis=0)
        den = float(np.sqrt(sums[0] * sums[1]))
        ncrs = self._fourierMaps()[0].header.ncrs
        return {"grid_c": int(ncrs[0]), "grid_r": int(ncrs[1]), "grid_s": int(ncrs[2]), "d_min": float(table["d_min"][-1]), "num_shells": int(nShells),
                "fsc_05_resolution": self.fscResolution(0.5, nShells), "fsc_0143_resolution": self.fscResolution(0.143, nShells),
                "overall_fsc": float(sums[2]) / den if den > 0 else None, "overall_scale": float(sums[2] / sums[1]) if sums[1] > 0 else None}

    fourierShellHeader = ["shell", "d_max", "d_min", "n", "power", "power_model", "fsc", "phase_cosine", "scale"]

    def calculateFourierShells(self, nShells=20):
        """One row per resolution shell (``fourierShellHeader``) of ``modelShellTable``; None where a value is undefined."""
        t = self.modelShellTable(nShells)
        clean = lambda v: [None if x != x else float(x) for x in np.asarray(v, dtype=np.float64).tolist()]
        return self._rows(list(range(len(t["n"]))), clean(t["d_max"]), clean(t["d_min"]), [int(v) for v in t["n"]], clean(t["power"]), clean(t["powerOther"]), clean(t["fsc"]),
                          clean(t["phaseCosine"]), clean(t["scale"]))

    # ---- masks of the whole cell: molecule, solvent, and the flat bulk-solvent model (no reference counterpart) ----
    def _maskAtoms(self, header, extra=0.0):
        """(xyz, radii) of every atom copy whose mask sphere (``ccp4.MASK_VDW`` by ``atom.element``, plus ``extra``) reaches the unit cell of
        ``header``: the atoms ``_cellAtoms`` keeps, copied the same way."""
        _requireParams()
        cols = _structure.columns(self.biopdbObj)
        names = cols.pair_names
        electrons = _pairTables(names, max(len(names), 1))["electrons"][cols.pair_of_atom] if len(cols.coord) else np.zeros(0)
        keep = ~np.isnan(electrons) & (cols.occupancy != 0) if len(cols.coord) else np.zeros(0, dtype=bool)
        radii = ccp4.maskRadii([getattr(atom, "element", "") or "" for atom in cols.atoms])[keep] if len(cols.coord) else np.zeros(0)
        xyz = np.asarray(cols.coord, dtype=np.float64).reshape(-1, 3)[keep]
        copies, rows = self._cellCopies(header, xyz, (float(radii.max()) if len(radii) else 0.0) + float(extra))
        return copies, radii[rows]

    @property
    def moleculeMaskObj(self):
        """1.0 inside the van der Waals spheres of the model's atoms and their symmetry mates, 0.0 outside, on the whole-cell grid of
        ``_fourierMaps`` (``DensityMatrix.atomMask``); resident."""
        if "moleculeMask" not in self._local:
            observed = self._fourierMaps()[0]
            xyz, radii = self._maskAtoms(observed.header)
            self._local["moleculeMask"] = observed.atomMask(xyz, radii)
        return self._local["moleculeMask"]

    @property
    def solventMaskObj(self):
        """1.0 in the bulk solvent of the whole cell, 0.0 in the molecule (``DensityMatrix.solventMask`` with the module's ``maskProbe`` and
        ``maskShrink``); resident."""
        if "solventMask" not in self._local:
            observed = self._fourierMaps()[0]
            xyz, radii = self._maskAtoms(observed.header, maskProbe)
            self._local["solventMask"] = observed.solventMask(xyz, radii, probe=maskProbe, shrink=maskShrink)
        return self._local["solventMask"]

    def _wholeCellDiff(self):
        """The Fo-Fc map on the grid of ``_fourierMaps``."""
        if "fourierDiff" not in self._local:
            header = self.densityObj.header
            if all(ccp4.isFourierSize(n) for n in header.crsInterval):
                self._local["fourierDiff"] = self.expandedDiffDensityObj
            else:
                self._local["fourierDiff"] = self.diffDensityObj.symmetryExpanded([np.asarray(m, dtype=np.float64) for m in self.pdbObj.header.rotationMats],
                                                                                  header=ccp4.fourierHeader(header), order=3)
        return self._local["fourierDiff"]

    def maskSummary(self):
        """The solvent fraction of the cell, mean and standard deviation of the 2Fo-Fc and Fo-Fc maps in the solvent and in the protein (the
        complement of the solvent mask), and ``solvent_noise``: the Fo-Fc sigma of the solvent, a noise estimate from where there is no model --
        ``partitionSummary``'s ``unowned_std`` asks the same of a distance to atom centres."""
        solvent = self.solventMaskObj
        protein = solvent.spread(np.zeros((1, 3), dtype=np.int32), np.array([1.0, 0.0], dtype=np.float32), 0.5, below=True)
        observed, diff = self._fourierMaps()[0], self._wholeCellDiff()
        n_solvent = observed.maskStats(solvent)[0]
        n_protein = observed.maskStats(protein)[0]
        out = {"cell_voxels": n_solvent + n_protein, "solvent_voxels": n_solvent, "solvent_fraction": n_solvent / max(n_solvent + n_protein, 1)}
        for region, mask in (("solvent", solvent), ("protein", protein)):
            for name, dm in (("density", observed), ("diff", diff)):
                _, mean, std = dm.maskStats(mask)
                out["%s_%s_mean" % (region, name)], out["%s_%s_std" % (region, name)] = mean, std
        out["solvent_noise"] = out["solvent_diff_std"]
        return out

    def maskedModelShellTable(self, nShells=20, width=3.0):
        """``modelShellTable`` with both whole-cell maps multiplied by the soft molecule mask: 1 inside the molecule, a raised cosine of
        ``width`` Angstrom outside it (``DensityMatrix.maskedBy``) -- the solvent region, where the model has nothing, stays out of the FSC."""
        key = ("maskedShells", int(nShells), float(width))
        if key not in self._local:
            observed, model = self._fourierMaps()
            mask = self.moleculeMaskObj
            self._local[key] = observed.maskedBy(mask, 0.0, width).shellStats(model.maskedBy(mask, 0.0, width), nShells)
        return self._local[key]

    def bulkSolventFit(self, bGrid=(20, 35, 50, 65, 80), nShells=20):
        """The flat bulk-solvent model Fo ~ a Fc + b S_B fitted over all shells: S_B is the spectrum of the solvent mask under
        ``ccp4.bFactorTable(B)``; for every B of ``bGrid`` the three pairwise shell sums of (Fo, Fc), (Fo, S_B) and (Fc, S_B) give the 2 x 2
        normal equations and the residual (``flatSolventFit``: host arithmetic on shell sums), and the B of the least residual wins.  A dict
        ``k_sol`` = b / a, ``b_sol``, ``scale`` = a, ``residual``, ``residuals`` (one per B), ``fsc_before`` / ``fsc_after`` per shell and the
        shells' ``d_max`` / ``d_min``.  Fo is the 2Fo-Fc map of the whole cell, Fc the model of ``_fourierMaps``."""
        key = ("bulkSolvent", tuple(float(b) for b in bGrid), int(nShells))
        if key not in self._local:
            observed, model = self._fourierMaps()
            fo, fc, s = observed.fourier(), model.fourier(), self.solventMaskObj.fourier()
            edges = ccp4.shellEdges(observed.header, nShells)
            s2Max = ccp4.maxS2(observed.header)
            base = fo.shells(fc, edges=edges)
            oo, cc, oc = base["sums"][:, 0], base["sums"][:, 1], base["sums"][:, 2]
            best, residuals = None, []
            for B in key[1]:
                sb = s.scaled(ccp4.bFactorTable(B, s2Max), s2Max)
                with_fo, with_fc = fo.shells(sb, edges=edges)["sums"], fc.shells(sb, edges=edges)["sums"]
                fit = flatSolventFit(oo, cc, with_fo[:, 1], oc, with_fo[:, 2], with_fc[:, 2])
                residuals.append(fit["residual"])
                if best is None or fit["residual"] < best[1]["residual"]:
                    best = (B, fit)
            B, fit = best
            self._local[key] = {"k_sol": fit["kSol"], "b_sol": B, "scale": fit["scale"], "residual": fit["residual"], "residuals": residuals,
                                "fsc_before": fit["fscBefore"], "fsc_after": fit["fscAfter"], "d_max": base["d_max"], "d_min": base["d_min"], "n": base["n"]}
        return self._local[key]

    def modelWithSolventObj(self, bGrid=(20, 35, 50, 65, 80), nShells=20):
        """The model plus the fitted bulk solvent on the whole-cell grid: combine(model, inverse(S_B), k_sol); resident."""
        fit = self.bulkSolventFit(bGrid, nShells)
        key = ("modelWithSolvent", fit["b_sol"], fit["k_sol"])
        if key not in self._local:
            observed, model = self._fourierMaps()
            s2Max = ccp4.maxS2(observed.header)
            smooth = self.solventMaskObj.fourier().scale(ccp4.bFactorTable(fit["b_sol"], s2Max), s2Max).toMap()
            self._local[key] = ccp4.DensityMatrix.fromDeviceMap(model.header, model.origin, type(model._map).combine(model._map, smooth._map, fit["k_sol"]), model.pdbid, model._ctx)
        return self._local[key]

    def solventShellTable(self, nShells=20):
        """``modelShellTable`` against ``modelWithSolventObj()``."""
        key = ("solventShells", int(nShells))
        if key not in self._local:
            self._local[key] = self._fourierMaps()[0].shellStats(self.modelWithSolventObj(nShells=nShells), nShells)
        return self._local[key]

    maskShellHeader = ["shell", "d_max", "d_min", "n", "fsc", "fsc_masked", "fsc_with_solvent"]

    def calculateMaskShells(self, nShells=20):
        """One row per resolution shell (``maskShellHeader``): the map-model FSC without a mask, inside the soft molecule mask, and with the fitted
        bulk solvent added to the model; None where a value is undefined."""
        plain, masked, solvent = self.modelShellTable(nShells), self.maskedModelShellTable(nShells), self.solventShellTable(nShells)
        clean = lambda v: [None if x != x else float(x) for x in np.asarray(v, dtype=np.float64).tolist()]
        return self._rows(list(range(len(plain["n"]))), clean(plain["d_max"]), clean(plain["d_min"]), [int(v) for v in plain["n"]], clean(plain["fsc"]), clean(masked["fsc"]),
                          clean(solvent["fsc"]))


maskProbe = 1.11         # DensityMatrix.solventMask's defaults: the atoms are grown by the probe, the molecule shrunk back by a ball
maskShrink = 0.9


def flatSolventFit(oo, cc, ss, oc, os_, cs):
    """The least-squares fit Fo ~ a Fc + b S over all shells from per-shell sums: ``oo``, ``cc``, ``ss`` = sum |Fo|^2, |Fc|^2, |S|^2 and ``oc``,
    ``os_``, ``cs`` = Re sum Fo Fc*, Fo S*, Fc S*.  The 2 x 2 normal equations [[CC, CS], [CS, SS]] (a, b) = (OC, OS) over the totals; where S
    vanishes or is parallel to Fc, a scale alone (b = 0).  A dict ``scale`` = a, ``b``, ``kSol`` = b / a, ``residual`` = sum |Fo - a Fc - b S|^2
    from the same sums, and per shell ``fscBefore`` (Fo against Fc) and ``fscAfter`` (Fo against a Fc + b S); NaN where a denominator is 0."""
    oo, cc, ss, oc, os_, cs = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (oo, cc, ss, oc, os_, cs))
    OO, CC, SS, OC, OS, CS = (math.fsum(v.tolist()) for v in (oo, cc, ss, oc, os_, cs))
    det = CC * SS - CS * CS
    if SS > 0 and det > 1e-12 * CC * SS:
        a, b = (OC * SS - OS * CS) / det, (OS * CC - OC * CS) / det
    else:
        a, b = (OC / CC if CC > 0 else float("nan")), 0.0
    residual = OO - 2.0 * a * OC - 2.0 * b * OS + a * a * CC + 2.0 * a * b * CS + b * b * SS
    with np.errstate(divide="ignore", invalid="ignore"):
        before = np.where(oo * cc > 0, oc / np.sqrt(oo * cc), np.nan)
        fitted = a * a * cc + 2.0 * a * b * cs + b * b * ss
        after = np.where(oo * fitted > 0, (a * oc + b * os_) / np.sqrt(oo * fitted), np.nan)
    return {"scale": a, "b": b, "kSol": b / a if a else float("nan"), "residual": residual, "fscBefore": before, "fscAfter": after}
