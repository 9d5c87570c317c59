"""CCP4 map object model on top of the MI355X voxel kernels.

Mirrors the reference's ``pdb_eda/ccp4.py`` API surface (``read``/``parse``,
``DensityHeader``, ``DensityMatrix``, ``DensityBlob``) so that
``singleStructure``/``multipleStructures``-style drivers work unchanged, but every
per-voxel operation (the reference's ``utils.*`` calls at ccp4.py:375-573) is executed
by ``libpdbeda_hip.so`` through the C-ABI in ``include/pdbeda.h``.  The parser is the
drop-in boundary named in BASELINE.json: it hands the raw [s][r][c] float32 grid and
the unit-cell basis to :func:`pdb_eda_amd._native.map_upload`.

There is no CPU fallback: constructing a ``DensityMatrix`` without the HIP library /
a GPU raises.
"""
import collections.abc
import math
import os
import sys

import numpy as np

from . import _native

__all__ = ["read", "parse", "read_grid", "DensityHeader", "DensityMatrix", "DensityBlob"]


def read(ccp4Filename, pdbid=None, verbose=False, ctx=None, lazy=False):
    """``ccp4.read`` (ref ccp4.py:58-74); ``ctx``: the context (= stream) the map becomes resident on.

    An uncompressed mode-2 file goes from the page cache to HBM through the library's upload engine
    (``pdbeda_map_upload_file``): only the header is parsed here, and ``DensityMatrix.density`` is fetched back on demand.
    ``lazy``: the header is read and the file's size checked now, the grid goes to HBM when something first asks for it
    (``DensityMatrix.resident`` tells) -- the Fo-Fc map of an entry whose analysis never looks at difference density (every
    record of ``pdb_eda multiple``, multipleStructures.py:320-356, reads its header only) then costs 1 KiB instead of a 32 MB
    upload.  A file that needs the parser (other modes, odd sizes) is read at once either way."""
    if not pdbid:
        pdbid = ccp4Filename
    with open(ccp4Filename, "rb") as fileHandle:
        head = fileHandle.read(1024)
        header = DensityHeader.fromFileHeader(head) if len(head) == 1024 else None
        n_bytes = 4 * header.ncrs[0] * header.ncrs[1] * header.ncrs[2] if header is not None else 0
        direct = header is not None and header.mode == 2 and n_bytes > 0 and os.fstat(fileHandle.fileno()).st_size == 1024 + header.symmetryBytes + n_bytes
        if not direct:
            fileHandle.seek(0)
            return parse(fileHandle, pdbid, verbose, ctx=ctx)
        assert header.xlength != 0.0 or header.ylength != 0.0 or header.zlength != 0.0, \
            "Error: Cell dimensions are all 0, Map file will not align with other structures"
        header.symmetry = fileHandle.read(header.symmetryBytes)
    ctx = ctx if ctx is not None else _native.default_context()
    swapped = header.endian != ("<" if sys.byteorder == "little" else ">")
    offset, geometry = 1024 + header.symmetryBytes, header.geometry()
    if lazy:
        dm = DensityMatrix.fromDeviceMap(header, header.origin, None, pdbid, ctx)
        dm._map_loader = lambda: _native.DeviceMap.from_file(ctx, ccp4Filename, offset, swapped, geometry)
        return dm
    return DensityMatrix.fromDeviceMap(header, header.origin, _native.DeviceMap.from_file(ctx, ccp4Filename, offset, swapped, geometry), pdbid, ctx)


def read_grid(handle):
    """Header + float32 grid view of a CCP4 stream (no device work): the SURVEY 8f-1 fast path.

    The reference unpacks every float into a Python tuple (``struct.unpack``, ccp4.py:123-124,
    0.93 s at 128^3); here the payload is viewed with ``np.frombuffer`` (both endiannesses,
    symmetry records skipped).  The reference's interval / axis "fix-ups" (ccp4.py:95-118) can
    never fire because of operator precedence (Q8) and are not reproduced; its one live check is.
    """
    raw = handle.read() if hasattr(handle, "read") else bytes(handle)
    header = DensityHeader.fromFileHeader(raw[:1024])
    assert header.xlength != 0.0 or header.ylength != 0.0 or header.zlength != 0.0, \
        "Error: Cell dimensions are all 0, Map file will not align with other structures"
    body = memoryview(raw)[1024:]
    header.symmetry = bytes(body[:header.symmetryBytes])
    payload = body[header.symmetryBytes:]
    grid = np.frombuffer(payload, dtype=header.endian + "f4", count=len(payload) // 4)
    return header, grid


def parse(handle, pdbid, verbose=False, ctx=None):
    """``ccp4.parse`` (ref ccp4.py:77-127): the grid goes straight to HBM."""
    header, grid = read_grid(handle)
    return DensityMatrix(header, header.origin, grid, pdbid, ctx=ctx)


def _libm_fma():
    """libm's fma (correctly rounded, IEEE 754): Python 3.10 has no math.fma."""
    import ctypes
    import ctypes.util
    try:
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fma
        fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double] * 3
        return fn if fn(3.0, 5.0, 7.0) == 22.0 else None
    except (OSError, AttributeError):
        return None


_fma_c = _libm_fma()


def _fma(a, b, c):
    """a * b + c with ONE rounding.  libm's when it loads (a header costs twelve of these: exact rational arithmetic took 0.1 ms of a
    pool entry's 1.2 ms of Python), else by exact rational arithmetic -- the same value either way."""
    if _fma_c is not None:
        return _fma_c(float(a), float(b), float(c))
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _dot3(mat, vec):
    """3x3 . 3 as numpy/OpenBLAS evaluates it in the reference environment:
    fma(a2, v2, fma(a0, v0, a1*v1)) per row (pinned bit-exactly by tests/golden)."""
    out = np.zeros(3, dtype=np.float64)
    for i in range(3):
        row = [float(x) for x in mat[i]]
        out[i] = _fma(row[2], vec[2], _fma(row[0], vec[0], row[1] * float(vec[1])))
    return out


def sphereLattice(n):
    """The spherical Fibonacci lattice of ``n`` unit vectors, (n, 3) float64: z_j = 1 - (2j + 1) / n, phi_j = j pi (3 - sqrt 5),
    u_j = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z).  The fixed sample directions of the Q-scores."""
    j = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * j + 1.0) / float(n)
    phi = j * (np.pi * (3.0 - np.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def _quaternionMatrices(q):
    """(n, 4) unit quaternions (x, y, z, w) -> (n, 3, 3) rotation matrices (rows orthonormal to a few 1e-16, determinant +1)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    out = np.empty((len(q), 3, 3), dtype=np.float64)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)
    out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = 2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)
    out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = 2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)
    return out


def rotationLattice(n):
    """``n`` rotation matrices, (n, 3, 3) float64, from a deterministic near-uniform lattice on SO(3): the super-Fibonacci spiral of unit
    quaternions (Alexa, CVPR 2022).  For i = 0 .. n-1 with s = i + 1/2, t = s / n, d = 2 pi s: q = (sqrt(t) sin(d / sqrt 2), sqrt(t) cos(d / sqrt 2),
    sqrt(1 - t) sin(d / psi), sqrt(1 - t) cos(d / psi)) as (x, y, z, w), psi = 1.533751168755204288118041 (the root of psi^4 = psi + 4), normalised
    once more in fp64.  No table and no random draw: the same matrices on every host.  Index 0 is NOT the identity: it is the first point of
    the spiral (for n = 1 a rotation by about 142 degrees); list the identity yourself where a search must contain it."""
    n = int(n)
    s = np.arange(n, dtype=np.float64) + 0.5
    t, d = s / float(max(n, 1)), 2.0 * np.pi * s
    r, big = np.sqrt(t), np.sqrt(1.0 - t)
    alpha, beta = d / np.sqrt(2.0), d / 1.533751168755204288118041
    q = np.stack([r * np.sin(alpha), r * np.cos(alpha), big * np.sin(beta), big * np.cos(beta)], axis=1)
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    return _quaternionMatrices(q)


def rotationsNear(R, angle, n):
    """``n`` rotations within ``angle`` (radians) of the rotation ``R``, (n, 3, 3), deterministic, ``R`` itself first.  Entry j >= 1 is D_j R: D_j
    turns by angle * (j / (n - 1))^(1/3) (the radii that fill a ball evenly) about direction j - 1 of ``sphereLattice(n - 1)``, as a unit
    quaternion, so the angle between entry j and ``R`` is exactly D_j's."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    n = int(n)
    if n <= 1:
        return R[None, :, :].copy()
    axes = sphereLattice(n - 1)
    theta = float(angle) * np.cbrt(np.arange(1, n, dtype=np.float64) / float(n - 1))
    q = np.concatenate([axes * np.sin(0.5 * theta)[:, None], np.cos(0.5 * theta)[:, None]], axis=1)
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    return np.concatenate([R[None, :, :], np.einsum("nij,jk->nik", _quaternionMatrices(q), R)])


def rotationAngle(a, b):
    """The angle (radians) of the rotation that carries ``a`` to ``b`` (3x3 each; ``a`` may be (n, 3, 3))."""
    trace = np.einsum("...ij,ij->...", np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(3, 3))
    return np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0))


def fragmentFrame(xyz, weights=None):
    """A rigid fragment in its own frame: a dict ``xyz`` (n, 3: the coordinates relative to the weighted centroid, the pivot of its rotations),
    ``weights`` (n,; ones when None), ``centroid`` (3,) and ``radius`` (max_a sqrt((x x + y y) + z z): what ``pdbeda_pose_scores`` sizes a centre's
    box by).  Weights that sum to zero fall back to the plain centroid."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    w = np.ones(len(xyz)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(xyz):
        raise ValueError("weights must have one value per atom")
    total = float(w.sum())
    centroid = (xyz * w[:, None]).sum(axis=0) / total if total != 0.0 else xyz.mean(axis=0)
    rel = xyz - centroid
    return {"xyz": rel, "weights": w, "centroid": centroid, "radius": float(np.sqrt((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]).max()) if len(rel) else 0.0}


_fmaElementwise = np.frompyfunc(_fma, 3, 1)


def placeFragment(frame, centre, R):
    """The coordinates (n, 3) of the pose (``centre``, ``R``) of a ``fragmentFrame`` (or of an (n, 3) array of pivot-relative coordinates),
    evaluated as the device evaluates them: p[i] = centre[i] + fma(R[i][2], x[2], fma(R[i][0], x[0], R[i][1] * x[1])), the add unfused."""
    x = np.asarray(frame["xyz"] if isinstance(frame, dict) else frame, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    out = np.empty_like(x)
    for i in range(3):
        dot = _fmaElementwise(R[i, 2], x[:, 2], _fmaElementwise(R[i, 0], x[:, 0], R[i, 1] * x[:, 1])).astype(np.float64) if len(x) else 0.0
        out[:, i] = c[i] + dot
    return out


def qScoreTables(sigma=0.6, step=0.1, nShells=21, nPoints=8, nLevels=4):
    """What the host hands ``pdbeda_atom_qscores``: (ref, unit_pts, level_offsets).  ref[k] = exp(-0.5 (k step32 / sigma)^2) with
    step32 = float(float32(step)), the radius the device uses; level l is ``sphereLattice(nPoints * 2**l)``."""
    step32 = float(np.float32(step))
    ref = np.exp(-0.5 * (np.arange(int(nShells), dtype=np.float64) * step32 / float(sigma)) ** 2)
    levels = [sphereLattice(int(nPoints) * 2 ** l) for l in range(int(nLevels))]
    offsets = np.concatenate([[0], np.cumsum([len(level) for level in levels])]).astype(np.int32)
    return ref, np.concatenate(levels), offsets


MODEL_MIN_B = 10.0       # B' never falls below this: sigma = sqrt(B' / (8 pi^2)) >= 0.36 A, which a 0.5 .. 1 A grid still samples
MODEL_N_SIGMA = 4.0      # the cut-off of an atom in sigmas: 0.11 % of its electrons lie beyond it, its last term is exp(-8) = 3.4e-4 of the peak


def gaussianAtomTerms(electrons, bfactors, occupancies, blur=0.0, minB=MODEL_MIN_B):
    """The single-Gaussian point-atom model that ``DensityMatrix.modelDensity`` takes: (amp, expo, bEff), (n,) float64 each.
    B' = max(B + blur, minB); rho(d) = amp exp(-expo d^2) with amp = occ Z (4 pi / B')^(3/2) and expo = 4 pi^2 / B' -- the Fourier
    transform of Z exp(-B' s^2 / 4), which integrates to occ Z electrons.  ``minB`` (default 10 A^2) keeps an atom wider than the grid:
    below it the Gaussian (sigma < 0.36 A) falls between the voxels of a 0.5 - 1 A grid and the sum over voxels no longer finds its
    electrons; ``blur`` adds to every B (a map sharpened or blurred by as much).  The kernel takes up to six terms per atom, so a caller
    with form-factor tables passes its own (n, n_terms) arrays instead; none are shipped."""
    z = np.asarray(electrons, dtype=np.float64).reshape(-1)
    b = np.maximum(np.asarray(bfactors, dtype=np.float64).reshape(-1) + float(blur), float(minB))
    occ = np.asarray(occupancies, dtype=np.float64).reshape(-1)
    return occ * z * (4.0 * np.pi / b) ** 1.5, 4.0 * np.pi ** 2 / b, b


def modelRadii(bEff, nSigma=MODEL_N_SIGMA):
    """The cut-off radius of every atom of ``gaussianAtomTerms``: float32(nSigma sqrt(B' / (8 pi^2))), ``nSigma`` standard deviations of
    its Gaussian (default 4: erfc(4 / sqrt 2) + sqrt(2 / pi) 4 exp(-8) = 0.11 % of the electrons lie outside)."""
    return (float(nSigma) * np.sqrt(np.asarray(bEff, dtype=np.float64) / (8.0 * np.pi ** 2))).astype(np.float32)


def gaussianAtomGradients(moments, electrons, bfactors, occupancies, blur=0.0, minB=MODEL_MIN_B):
    """The chain rule of ``gaussianAtomTerms``' one-Gaussian model on the sums of ``DensityMatrix.atomMoments``: the derivatives of
    F = sum_v w(v) rho_a(v) with respect to the atom's position, B and occupancy, as a dict ``dXyz`` (n, 3), ``dB`` and ``dOcc`` (n,).
    ``moments`` is (n, 5) or (n, 1, 5): M0, Mx, My, Mz, M2 of term 0, the offsets being voxel minus atom.  With rho = amp exp(-expo d^2),
    amp = occ Z (4 pi / B')^(3/2), expo = 4 pi^2 / B':  dXyz = 2 expo amp (Mx, My, Mz);  dOcc = Z (4 pi / B')^(3/2) M0 (amp / occ without
    the division: an occupancy of 0 has a derivative);  dB = amp (-1.5 M0 / B' + 4 pi^2 M2 / B'^2), and 0 where B + blur < minB: the
    clamp B' = max(B + blur, minB) is flat there."""
    z = np.asarray(electrons, dtype=np.float64).reshape(-1)
    n = len(z)
    m = np.asarray(moments, dtype=np.float64).reshape(n, -1, 5)[:, 0, :] if n else np.zeros((0, 5))
    raw = np.asarray(bfactors, dtype=np.float64).reshape(-1) + float(blur)
    b = np.maximum(raw, float(minB))
    occ = np.asarray(occupancies, dtype=np.float64).reshape(-1)
    unit = z * (4.0 * np.pi / b) ** 1.5
    amp, expo = occ * unit, 4.0 * np.pi ** 2 / b
    dB = amp * (-1.5 * m[:, 0] / b + 4.0 * np.pi ** 2 * m[:, 4] / (b * b))
    return {"dXyz": (2.0 * expo * amp)[:, None] * m[:, 1:4], "dB": np.where(raw < float(minB), 0.0, dB), "dOcc": unit * m[:, 0]}


def gaussianAtomCurvatures(electrons, bfactors, occupancies, unitVolume, blur=0.0, minB=MODEL_MIN_B):
    """The diagonal Gauss-Newton curvature of sum_v rho_a(v)^2 / 2 for an ISOLATED Gaussian atom, from closed-form integrals divided by
    the voxel volume: with G = (pi / (2 expo))^(3/2), int (d rho / d x)^2 = expo amp^2 G, int (d rho / d B)^2 = (15 / 16) (amp / B')^2 G,
    int (d rho / d occ)^2 = (amp / occ)^2 G.  A dict ``xyz``, ``b``, ``occ`` of (n,) arrays.  Overlap with neighbours and the ragged
    cut-off are ignored: the step that divides by these is checked against the target before it is taken."""
    z = np.asarray(electrons, dtype=np.float64).reshape(-1)
    b = np.maximum(np.asarray(bfactors, dtype=np.float64).reshape(-1) + float(blur), float(minB))
    occ = np.asarray(occupancies, dtype=np.float64).reshape(-1)
    unit = z * (4.0 * np.pi / b) ** 1.5
    amp, expo = occ * unit, 4.0 * np.pi ** 2 / b
    g = (np.pi / (2.0 * expo)) ** 1.5 / float(unitVolume)
    return {"xyz": expo * amp * amp * g, "b": (15.0 / 16.0) * (amp / b) ** 2 * g, "occ": unit * unit * g}


def foldImageGradients(grad, rows, rotations, nAtoms):
    """The gradients of image atoms brought back to the atoms they are copies of: image k is atom ``rows[k]`` under x -> R_k x + t_k, so its
    positional gradient comes back through the TRANSPOSE of R_k; dB and dOcc simply add.  ``grad`` is the dict of
    ``gaussianAtomGradients`` over the images, ``rotations`` (m, 3, 3); the result is that dict over ``nAtoms`` atoms.  Added in the order
    of the images (np.add.at): one order, one result."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    rot = np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)
    back = np.einsum("kji,kj->ki", rot, np.asarray(grad["dXyz"], dtype=np.float64).reshape(-1, 3))
    out = {"dXyz": np.zeros((nAtoms, 3)), "dB": np.zeros(nAtoms), "dOcc": np.zeros(nAtoms)}
    np.add.at(out["dXyz"], rows, back)
    np.add.at(out["dB"], rows, np.asarray(grad["dB"], dtype=np.float64))
    np.add.at(out["dOcc"], rows, np.asarray(grad["dOcc"], dtype=np.float64))
    return out


def gaussNewtonStep(gradT, curvature, scale, what, maxShift, maxDeltaB=20.0, damping=1.0):
    """The damped diagonal Gauss-Newton step against the gradient of T: delta = -damping g / (scale^2 curvature), 0 where the curvature is.
    A dict ``xyz`` (n, 3; the vector is shortened to ``maxShift``), ``b`` (capped at +-maxDeltaB) and ``occ``; zeros for what is not in
    ``what``."""
    n = len(gradT["dB"])
    s2 = float(scale) ** 2

    def ratio(g, h):
        h = s2 * np.asarray(h, dtype=np.float64)
        return np.where(h > 0, -float(damping) * g / np.where(h > 0, h, 1.0), 0.0)

    step = {"xyz": np.zeros((n, 3)), "b": np.zeros(n), "occ": np.zeros(n)}
    if "xyz" in what:
        d = ratio(gradT["dXyz"], np.asarray(curvature["xyz"])[:, None])
        length = np.sqrt((d * d).sum(axis=1))
        step["xyz"] = d * np.where(length > maxShift, maxShift / np.where(length > 0, length, 1.0), 1.0)[:, None]
    if "b" in what:
        step["b"] = np.clip(ratio(gradT["dB"], curvature["b"]), -float(maxDeltaB), float(maxDeltaB))
    if "occ" in what:
        step["occ"] = ratio(gradT["dOcc"], curvature["occ"])
    return step


def gaussianTaps(sigmaVoxels, truncate=4.0):
    """The weights of a Gaussian of ``sigmaVoxels`` grid steps for ``DensityMatrix.filtered`` / ``localStats``: radius int(truncate sigma +
    0.5), exp(-x^2 / 2 sigma^2) divided by its sum -- ``scipy.ndimage.gaussian_filter``'s own weights.  sigma = 0 gives [1.0]."""
    sigma = float(sigmaVoxels)
    if not (sigma >= 0.0 and math.isfinite(sigma)) or not (float(truncate) >= 0.0 and math.isfinite(float(truncate))):
        raise ValueError("gaussianTaps: sigma and truncate must be finite and >= 0")
    radius = int(float(truncate) * sigma + 0.5)
    if radius == 0 or sigma == 0.0:
        return np.ones(1, dtype=np.float64)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def boxTaps(halfWidth):
    """2 halfWidth + 1 equal weights: the moving average (``scipy.ndimage.uniform_filter`` of that size)."""
    h = int(halfWidth)
    if h < 0:
        raise ValueError("boxTaps: halfWidth must be >= 0")
    return np.full(2 * h + 1, 1.0 / (2 * h + 1), dtype=np.float64)


FILTER_MAX_RADIUS = _native.FILTER_MAX_RADIUS      # PDBEDA_FILTER_MAX_RADIUS of include/pdbeda.h


# -- coordinate operators and destination headers for ``DensityMatrix.resampled`` (host numpy; no reference counterpart) --
RESAMPLE_MAX_OPS = _native.RESAMPLE_MAX_OPS      # PDBEDA_RESAMPLE_MAX_OPS of include/pdbeda.h


def _operator(op):
    """An operator as a (3, 4) float64 array [R | t] (a 3 x 4 array, 12 numbers, or a row of ``PDBHeader.rotationMats``)."""
    return np.array(op, dtype=np.float64).reshape(3, 4)


def identityOperator():
    """[I | 0]: x -> x."""
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def invertOperator(op):
    """The operator that undoes ``op``: x -> R^-1 (x - t)."""
    op = _operator(op)
    inv = np.linalg.inv(op[:, :3])
    return np.hstack([inv, -inv.dot(op[:, 3:])])


def composeOperators(a, b):
    """``a`` after ``b``: x -> a(b(x))."""
    a, b = _operator(a), _operator(b)
    return np.hstack([a[:, :3].dot(b[:, :3]), a[:, :3].dot(b[:, 3:]) + a[:, 3:]])


def applyOperator(op, xyz):
    """``op`` on an (n, 3) array of coordinates."""
    op = _operator(op)
    return np.asarray(xyz, dtype=np.float64).reshape(-1, 3).dot(op[:, :3].T) + op[:, 3]


def kabschOperator(fromXyz, toXyz, weights=None):
    """(op, rmsd): the PROPER rotation and the shift with op(fromXyz) ~ toXyz in the (weighted) least-squares sense (Kabsch 1976), and
    the root-mean-square distance that is left.  Where the SVD's best orthogonal matrix is a reflection, the sign of the smallest
    singular direction is flipped: the result is always a rotation (det = +1)."""
    p, q = np.asarray(fromXyz, dtype=np.float64).reshape(-1, 3), np.asarray(toXyz, dtype=np.float64).reshape(-1, 3)
    if len(p) != len(q) or len(p) < 3:
        raise ValueError("kabschOperator takes two lists of the same three or more points")
    w = np.ones(len(p)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(p) or not (w >= 0).all() or not w.sum() > 0:
        raise ValueError("kabschOperator: one weight >= 0 per point, not all zero")
    w = w / w.sum()
    cp, cq = w.dot(p), w.dot(q)
    u, _, vt = np.linalg.svd(((p - cp) * w[:, None]).T.dot(q - cq))
    d = np.sign(np.linalg.det(vt.T.dot(u.T)))
    rot = vt.T.dot(np.diag([1.0, 1.0, d if d != 0 else 1.0])).dot(u.T)
    op = np.hstack([rot, (cq - rot.dot(cp)).reshape(3, 1)])
    return op, float(np.sqrt(w.dot(((applyOperator(op, p) - q) ** 2).sum(axis=1))))


def _headerFromFields(ncrs, crsStart, xyzInterval, xyzLength, angles, axes, spaceGroup=1):
    """A mode-2 DensityHeader without file, symmetry records or statistics, through the constructor."""
    t = tuple(int(v) for v in ncrs) + (2,) + tuple(int(v) for v in crsStart) + tuple(int(v) for v in xyzInterval) + tuple(float(v) for v in xyzLength) + \
        tuple(float(v) for v in angles) + tuple(int(v) for v in axes) + (0.0, 0.0, 0.0, int(spaceGroup), 0, 0) + (0.0,) * 27 + (b"M", b"A", b"P", b" ") + (0, 0.0, 0)
    return DensityHeader(t, b"", "<" if sys.byteorder == "little" else ">")


def cellHeader(header):
    """``header``'s cell and sampling with crsStart 0 and ncrs = crsInterval: the WHOLE unit cell, the destination of a symmetry expansion."""
    return _headerFromFields(header.crsInterval, (0, 0, 0), header.xyzInterval, header.xyzLength, (header.alpha, header.beta, header.gamma),
                             (header.col2xyz, header.row2xyz, header.sec2xyz), header.spaceGroup)


def boxHeader(centre, halfWidth, spacing):
    """An orthogonal P1 header (columns along x) whose stored box covers ``centre`` +- ``halfWidth`` (A; a number or one per axis) on a grid
    of ``spacing`` A: crsStart lies on the grid through the coordinate origin, the cell is twice the box along every axis (nothing of
    it wraps onto itself), and the cell lengths are float32 numbers -- they survive a CCP4 header --, so that the grid step is the
    spacing to within 2^-24 of it."""
    centre = np.asarray(centre, dtype=np.float64).reshape(3)
    half = np.broadcast_to(np.asarray(halfWidth, dtype=np.float64), (3,))
    step = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    if not (np.isfinite(centre).all() and (half >= 0).all() and np.isfinite(half).all() and (step > 0).all() and np.isfinite(step).all()):
        raise ValueError("boxHeader: a finite centre, halfWidth >= 0 and spacing > 0")
    start, ncrs, interval, length = [], [], [], []
    for k in range(3):
        n = int(math.ceil(2.0 * half[k] / step[k])) + 4      # (enough for any placement of the box on the grid)
        cell = float(np.float32(2 * n * step[k]))
        g = cell / (2 * n)
        pad = 1e-9 * (abs(centre[k]) + half[k] + 1.0)         # (above the rounding of the header's own origin and crs2xyzCoord)
        first, last = int(math.floor((centre[k] - half[k] - pad) / g)), int(math.ceil((centre[k] + half[k] + pad) / g))
        if last - first + 1 > n:
            raise ValueError("boxHeader: the box does not fit the grid it was sized for")
        start.append(first); ncrs.append(last - first + 1); interval.append(2 * n); length.append(cell)
    return _headerFromFields(ncrs, start, interval, length, (90.0, 90.0, 90.0), (1, 2, 3))


# -- reciprocal space: plannable sizes, the metric, shells and radial tables for ``DensityMatrix.fourier`` (host numpy; no reference counterpart) --
FFT_MAX_AXIS = _native.FFT_MAX_AXIS                  # PDBEDA_FFT_MAX_AXIS of include/pdbeda.h
SPECTRUM_MAX_TABLE = _native.SPECTRUM_MAX_TABLE      # PDBEDA_SPECTRUM_MAX_TABLE
SPECTRUM_MAX_SHELLS = _native.SPECTRUM_MAX_SHELLS    # PDBEDA_SPECTRUM_MAX_SHELLS


def isFourierSize(n):
    """Whether an axis of ``n`` indices can be transformed: n = 2^a 3^b 5^c 7^d, 1 <= n <= FFT_MAX_AXIS (pdbeda_fft_plan)."""
    n = int(n)
    if n < 1 or n > FFT_MAX_AXIS:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def fourierSize(n):
    """The next plannable length at or above ``n``; ValueError beyond FFT_MAX_AXIS."""
    k = max(int(n), 1)
    while k <= FFT_MAX_AXIS:
        if isFourierSize(k):
            return k
        k += 1
    raise ValueError("no plannable Fourier length at or above %d (the longest line is %d)" % (int(n), FFT_MAX_AXIS))


def fourierHeader(header):
    """The WHOLE unit cell of ``header`` sampled at the next plannable intervals (``fourierSize`` of every xyzInterval), crsStart 0: the
    destination of a tricubic ``resampled`` / ``symmetryExpanded`` when the cell's own sampling cannot be transformed.  A cell whose sampling
    is plannable gives ``cellHeader``'s grid."""
    interval = [fourierSize(v) for v in header.xyzInterval]
    return _headerFromFields([interval[a] for a in header.map2crs], (0, 0, 0), interval, header.xyzLength, (header.alpha, header.beta, header.gamma),
                             (header.col2xyz, header.row2xyz, header.sec2xyz), header.spaceGroup)


def reciprocalMetric(header):
    """The six numbers {m00, m11, m22, m01, m02, m12} of M = (B^T B)^-1 for the STORED BOX of ``header`` as the period: the columns of B are
    b_k = orthoMat[:, map2crs[k]] * ncrs[k] / crsInterval[k], k in crs order, and s^2 = h^T M h = 1 / d^2 for the frequency numbers h of a
    coefficient (what ``pdbeda_spectrum_scale`` / ``pdbeda_spectrum_shells`` take).  For a whole-cell map h are the Miller indices in crs order."""
    ortho = np.asarray(header.orthoMat, dtype=np.float64)
    b = np.stack([ortho[:, header.map2crs[k]] * (float(header.ncrs[k]) / float(header.crsInterval[k])) for k in range(3)], axis=1)
    m = np.linalg.inv(b.T.dot(b))
    return np.array([m[0, 0], m[1, 1], m[2, 2], 0.5 * (m[0, 1] + m[1, 0]), 0.5 * (m[0, 2] + m[2, 0]), 0.5 * (m[1, 2] + m[2, 1])], dtype=np.float64)


def _nyquist(header, metric):
    """The smallest |s| of the three axis Nyquist points (h = n / 2 along one axis): the resolution every direction of the box supports."""
    return min(0.5 * header.ncrs[k] * math.sqrt(metric[k]) for k in range(3))


def maxS2(header):
    """An upper bound of s^2 over the coefficients of the stored box: the largest over the eight corners h = +- n / 2, times 1 + 2^-20."""
    m = reciprocalMetric(header)
    best = 0.0
    for sr in (-1.0, 1.0):
        for ss in (-1.0, 1.0):
            h = (0.5 * header.ncrs[0], sr * 0.5 * header.ncrs[1], ss * 0.5 * header.ncrs[2])
            best = max(best, m[0] * h[0] * h[0] + m[1] * h[1] * h[1] + m[2] * h[2] * h[2] + 2.0 * (m[3] * h[0] * h[1] + m[4] * h[0] * h[2] + m[5] * h[1] * h[2]))
    return best * (1.0 + 2.0 ** -20)


def shellEdges(header, nShells, dMin=None, dMax=None):
    """nShells + 1 ascending edges of s^2 = 1 / d^2 in equal steps of s^3, i.e. shells of equal reciprocal volume, from 1 / dMax to 1 / dMin.
    dMin defaults to the Nyquist limit of the coarsest axis (the edge lies 2^-20 above it, so that the Nyquist coefficient is in the last
    shell whatever the rounding); dMax defaults to twice the longest axis period of the box, so the first edge is above 0 and F(000) is
    in no shell."""
    n = int(nShells)
    if n < 1 or n > SPECTRUM_MAX_SHELLS:
        raise ValueError("shellEdges: 1 .. %d shells" % SPECTRUM_MAX_SHELLS)
    m = reciprocalMetric(header)
    hi = _nyquist(header, m) * (1.0 + 2.0 ** -20) if dMin is None else 1.0 / float(dMin)
    lo = 0.5 * min(math.sqrt(m[k]) for k in range(3)) if dMax is None else 1.0 / float(dMax)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError("shellEdges: 0 < 1 / dMax < 1 / dMin is required")
    cubes = lo ** 3 + (hi ** 3 - lo ** 3) * (np.arange(n + 1, dtype=np.float64) / n)
    edges = np.cbrt(cubes) ** 2
    edges[0], edges[-1] = lo * lo, hi * hi
    return edges


def bFactorTable(B, s2Max, n=1024):
    """exp(-B s^2 / 4) at n equal steps of s^2 over [0, s2Max] for ``DensitySpectrum.scaled``: B > 0 blurs, B < 0 sharpens."""
    return np.exp(-0.25 * float(B) * np.linspace(0.0, float(s2Max), int(n)))


def resolutionTable(dMin=None, dMax=None, softness=0.1, s2Max=None, n=1024):
    """A raised-cosine window in s = 1 / d at n equal steps of s^2 over [0, s2Max]: 1 inside the band 1 / dMax <= s <= 1 / dMin and 0 outside,
    each edge s_c a half cosine from s_c (1 - softness / 2) to s_c (1 + softness / 2) (softness 0: a step).  s2Max defaults to the end of the
    upper roll-off (pass ``beyond=0``); with dMax alone (a high-pass) s2Max must be given (pass ``beyond=1``)."""
    soft = float(softness)
    if not (0.0 <= soft < 2.0):
        raise ValueError("resolutionTable: softness in [0, 2)")
    if dMin is None and dMax is None:
        raise ValueError("resolutionTable takes dMin, dMax or both")
    if s2Max is None:
        if dMin is None:
            raise ValueError("resolutionTable: a high-pass table needs s2Max")
        s2Max = ((1.0 + 0.5 * soft) / float(dMin)) ** 2 * (1.0 + 2.0 ** -20)
    s = np.sqrt(np.linspace(0.0, float(s2Max), int(n)))

    def lowpass(sc):
        a, b = sc * (1.0 - 0.5 * soft), sc * (1.0 + 0.5 * soft)
        if b <= a:
            return (s <= sc).astype(np.float64)
        return np.where(s <= a, 1.0, np.where(s >= b, 0.0, 0.5 * (1.0 + np.cos(np.pi * (np.clip(s, a, b) - a) / (b - a)))))
    g = np.ones_like(s)
    if dMin is not None:
        g = g * lowpass(1.0 / float(dMin))
    if dMax is not None:
        g = g * (1.0 - lowpass(1.0 / float(dMax)))
    return g


class DensityHeader(object):
    """CCP4 header + derived cell geometry (ref ccp4.py:130-316).

    The derived fields keep the reference's names and -- because they feed exact
    rounding decisions downstream (Q5) -- the reference's floating-point evaluation
    order, including the two library calls it makes (``np.linalg.inv``, ``np.dot``).
    """

    @classmethod
    def fromFileHeader(cls, fileHeader):
        mode_le = int.from_bytes(fileHeader[12:16], byteorder="little")
        endian = "<" if 0 <= mode_le <= 6 else ">"
        iw = np.frombuffer(fileHeader, dtype=endian + "i4", count=56)
        fw = np.frombuffer(fileHeader, dtype=endian + "f4", count=56)
        fields = [int(x) for x in iw[0:10]] + [float(x) for x in fw[10:16]] + [int(x) for x in iw[16:19]] + \
                 [float(x) for x in fw[19:22]] + [int(x) for x in iw[22:25]] + [float(x) for x in fw[25:52]] + \
                 [bytes(fileHeader[208 + k:209 + k]) for k in range(4)] + [int(iw[53]), float(fw[54]), int(iw[55])]
        labels = bytes(fileHeader[224:]).replace(b" ", b"")
        return cls(tuple(fields), labels, endian)

    def __init__(self, headerTuple, labels, endian):
        t = headerTuple
        self.ncrs = t[0:3]
        self.mode = t[3]
        self.endian = endian
        self.crsStart = t[4:7]
        self.nintervalX, self.nintervalY, self.nintervalZ = t[7], t[8], t[9]
        self.xlength, self.ylength, self.zlength = t[10], t[11], t[12]
        self.alpha, self.beta, self.gamma = t[13], t[14], t[15]
        self.col2xyz, self.row2xyz, self.sec2xyz = t[16], t[17], t[18]
        self.densityMin, self.densityMax, self.densityMean = t[19], t[20], t[21]
        self.spaceGroup = t[22]
        self.symmetryBytes = t[23]
        self.skewFlag = t[24]
        self.skewMat = t[25:34]
        self.skewTrans = t[34:37]
        self.futureUse = t[37:49]
        self.originEM = t[49:52]
        self.mapChar = t[52:56]
        self.machineStamp = t[56]
        self.rmsd = t[57]
        self.nLabel = t[58]
        self.labels = labels
        self.symmetry = b""

        self.mapSize = self.ncrs[0] * self.ncrs[1] * self.ncrs[2] * 4
        self.xyzLength = [self.xlength, self.ylength, self.zlength]
        self.xyzInterval = [self.nintervalX, self.nintervalY, self.nintervalZ]
        self.gridLength = [length / n for length, n in zip(self.xyzLength, self.xyzInterval)]

        axis_of = (self.col2xyz - 1, self.row2xyz - 1, self.sec2xyz - 1)      # crs axis -> xyz axis
        self.map2crs = list(axis_of)
        self.map2xyz = [0, 0, 0]                                              # xyz axis -> crs axis
        for crs_axis, xyz_axis in enumerate(axis_of):
            self.map2xyz[xyz_axis] = crs_axis
        self.crsInterval = [self.xyzInterval[a] for a in axis_of]

        # ref ccp4.py:240-253 (kept in the reference's operation order)
        a = np.pi / 180 * self.alpha
        b = np.pi / 180 * self.beta
        g = np.pi / 180 * self.gamma
        skew = np.sqrt(1 - np.cos(a) ** 2 - np.cos(b) ** 2 - np.cos(g) ** 2 + 2 * np.cos(a) * np.cos(b) * np.cos(g))
        self.unitVolume = self.xlength * self.ylength * self.zlength / self.nintervalX / self.nintervalY / self.nintervalZ * skew
        self.orthoMat = [[self.xlength, self.ylength * np.cos(g), self.zlength * np.cos(b)],
                         [0, self.ylength * np.sin(g), self.zlength * (np.cos(a) - np.cos(b) * np.cos(g)) / np.sin(g)],
                         [0, 0, self.zlength * skew / np.sin(g)]]
        self.deOrthoMat = np.linalg.inv(self.orthoMat)
        self.deOrthoMat[abs(self.deOrthoMat) < 1e-10] = 0.0

        self.emOrigin = not (self.futureUse[-3] == 0.0 and self.futureUse[-2] == 0.0 and self.futureUse[-1] == 0.0)
        self.origin = self._calculateOrigin()
        self.uniqueNcrs = [min(self.ncrs[k], self.crsInterval[k]) for k in range(3)]
        self.orthogonal = bool(self.alpha == self.beta == self.gamma == 90)

    def _calculateOrigin(self):
        """ref ccp4.py:272-286.  The reference's ``np.dot(orthoMat, frac)`` is evaluated in the
        accumulation order its BLAS uses in the reference environment (see ``_dot3``) so that the
        origin -- which every rounding decision downstream depends on -- is host independent."""
        if not self.emOrigin:
            return _dot3(self.orthoMat, [self.crsStart[self.map2xyz[i]] / self.xyzInterval[i] for i in range(3)])
        return [self.originEM[i] for i in range(3)]

    def xyz2crsCoord(self, xyzCoord):
        """ref ccp4.py:288-302 (host copy, used for single points; bulk work runs on the GPU)."""
        if self.orthogonal:
            grid = [int(round((xyzCoord[i] - self.origin[i]) / self.gridLength[i])) for i in range(3)]
        else:
            frac = np.dot(self.deOrthoMat, xyzCoord)
            grid = [int(round(frac[i] * self.xyzInterval[i])) - self.crsStart[self.map2xyz[i]] for i in range(3)]
        return [grid[self.map2crs[i]] for i in range(3)]

    def crs2xyzCoord(self, crsCoord):
        """ref ccp4.py:304-316."""
        if self.orthogonal:
            return [crsCoord[self.map2xyz[i]] * self.gridLength[i] + self.origin[i] for i in range(3)]
        return np.dot(self.orthoMat, [(crsCoord[self.map2xyz[i]] + self.crsStart[self.map2xyz[i]]) / self.xyzInterval[i]
                                      for i in range(3)])

    def crs2xyz_array(self, crs):
        """Vectorised crs -> xyz for host-side generators (not bit-pinned)."""
        crs = np.asarray(crs, dtype=np.float64)
        if self.orthogonal:
            return np.stack([crs[:, self.map2xyz[i]] * self.gridLength[i] + self.origin[i] for i in range(3)], axis=1)
        frac = np.stack([(crs[:, self.map2xyz[i]] + self.crsStart[self.map2xyz[i]]) / self.xyzInterval[i] for i in range(3)], axis=1)
        return frac.dot(np.asarray(self.orthoMat, dtype=np.float64).T)

    def geometry(self):
        """Pack the unit-cell basis for the C-ABI (``pdbeda_geometry``, include/pdbeda.h)."""
        if self.emOrigin:
            # Q6: with ORIGIN-record (EM) maps the reference's own sphere code degenerates
            # (list concatenation in cutils.pyx:239); such maps are rejected explicitly.
            raise ValueError("CCP4 maps that use the EM ORIGIN records are not supported (see DESIGN.md, Q6)")
        return _native.make_geometry(self.ncrs, self.crsStart, self.xyzInterval, self.map2xyz, self.map2crs,
                                     self.orthogonal, np.asarray(self.orthoMat, dtype=np.float64),
                                     np.asarray(self.deOrthoMat, dtype=np.float64),
                                     np.asarray(self.origin, dtype=np.float64), self.gridLength, self.unitVolume)


class DensitySpectrum(object):
    """The Fourier transform of a DensityMatrix, resident in HBM: the Hermitian half [ns][nr][nc / 2 + 1] of numpy's ``rfftn`` of the stored
    box, complex fp64 (``DensityMatrix.fourier``).  ``metric`` is ``reciprocalMetric`` of the map's header."""

    def __init__(self, densityMatrix, deviceSpectrum):
        self.densityMatrix = densityMatrix
        self.header = densityMatrix.header
        self._spec = deviceSpectrum
        self.metric = reciprocalMetric(self.header)
        self._scales = []

    @property
    def shape(self):
        """(ns, nr, nc // 2 + 1)."""
        return self._spec.shape

    def values(self):
        """The coefficients on the host: complex128 [ns][nr][nc // 2 + 1]."""
        return self._spec.download()

    def at(self, idx):
        """The coefficients at integer indices ``idx`` ((n, 3), crs order: column, row, section frequency): any integer, reduced modulo the
        axis; the missing half through the Hermitian mirror.  complex128 (n,)."""
        return self._spec.values(idx)

    def scale(self, table, s2Max, beyond=0.0):
        """Multiply every coefficient IN PLACE by g(s^2): ``table`` holds g at equal steps of s^2 over [0, s2Max], read by linear
        interpolation; ``beyond`` above s2Max (``pdbeda_spectrum_scale``).  Returns self."""
        table = np.array(table, dtype=np.float64).reshape(-1)
        self._spec.scale(self.metric, table, s2Max, beyond)
        self._scales.append((table, float(s2Max), float(beyond)))
        return self

    def scaled(self, table, s2Max, beyond=0.0):
        """A NEW spectrum: this one times g(s^2) (see ``scale``); this one is left as it is (the map is transformed again and the tables
        this spectrum has seen are applied in their order)."""
        out = DensitySpectrum(self.densityMatrix, self.densityMatrix._map.fft())
        for t, s2, b in self._scales:
            out.scale(t, s2, b)
        return out.scale(table, s2Max, beyond)

    def toMap(self):
        """The inverse transform as a device-made DensityMatrix on the header of the map this spectrum came from."""
        return self.densityMatrix._made(self._spec.inverse(self.densityMatrix._map))

    def shells(self, other=None, edges=None, nShells=20, dMin=None, dMax=None):
        """Sums over resolution shells (``pdbeda_spectrum_shells``): a dict of arrays per shell -- ``d_max`` and ``d_min`` (the shell's limits
        in Angstrom), ``n`` (coefficients of the full spectrum), ``power`` (mean |F|^2) and, with ``other`` (a DensitySpectrum of the same
        shape), ``powerOther``, ``fsc`` = Re sum(A conj B) / sqrt(sum |A|^2 sum |B|^2), ``phaseCosine`` (the cosine of the phase of sum(A conj B) over the STORED half with its weights:
        1 for maps that agree, below 1 when one is shifted against the other) and ``scale``
        (the least-squares k of self ~ k other: Re sum(A conj B) / sum |B|^2).  NaN where a denominator is 0.  ``edges`` are in s^2
        (default: ``shellEdges(header, nShells, dMin, dMax)``)."""
        edges = shellEdges(self.header, nShells, dMin, dMax) if edges is None else np.asarray(edges, dtype=np.float64).reshape(-1)
        count, sums = self._spec.shells(None if other is None else other._spec, self.metric, edges)
        saa, sbb, re, im = sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3]
        nan = np.full(len(count), np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            nf = count.astype(np.float64)
            out = {"d_max": 1.0 / np.sqrt(edges[:-1]), "d_min": 1.0 / np.sqrt(edges[1:]), "n": count,
                   "power": np.where(count > 0, saa / nf, np.nan)}
            if other is None:
                out.update({"powerOther": nan, "fsc": nan.copy(), "phaseCosine": nan.copy(), "scale": nan.copy()})
            else:
                den = np.sqrt(saa * sbb)
                mod = np.sqrt(re * re + im * im)
                out.update({"powerOther": np.where(count > 0, sbb / nf, np.nan), "fsc": np.where(den > 0, re / den, np.nan),
                            "phaseCosine": np.where(mod > 0, re / mod, np.nan), "scale": np.where(sbb > 0, re / sbb, np.nan)})
        out["sums"] = sums
        return out


class DensityMatrix(object):
    """A CCP4 map resident in HBM (ref ccp4.py:319-485).

    ``density`` stays available as a host float32 view for inspection, but no method
    computes from it; all methods call the C-ABI.
    """

    @classmethod
    def fromDeviceMap(cls, header, origin, device_map, pdbid, ctx):
        """A DensityMatrix around a map that already lives in HBM (``DeviceMap.combine`` / ``from_file``); ``density`` is
        downloaded on first use, for inspection."""
        self = cls.__new__(cls)
        self.pdbid, self.header, self.origin = pdbid, header, origin
        self._ctx, self._map = ctx, device_map
        self._density = None
        self._densityArray = None
        self._flatOf = None
        self._meanDensity = self._stdDensity = None
        self._totalAbsDensity = {}
        return self

    def __init__(self, header, origin, density, pdbid, ctx=None):
        self.pdbid = pdbid
        self.header = header
        self.origin = origin
        grid = np.asarray(density)
        if grid.dtype != np.float32 or not grid.dtype.isnative:
            grid = grid.astype(np.float32)
        self._density = np.ascontiguousarray(grid).reshape(header.ncrs[2], header.ncrs[1], header.ncrs[0])
        self._densityArray = None
        self._flatOf = None                 # another DensityMatrix whose flat array stands in for this one's (densityAnalysis.fc)
        self._ctx = ctx if ctx is not None else _native.default_context()
        self._map = _native.DeviceMap(self._ctx, self._density, header.geometry())
        self._meanDensity = None
        self._stdDensity = None
        self._totalAbsDensity = {}

    # the resident map: made on first use when the file was read lazily (``ccp4.read(..., lazy=True)``)
    @property
    def _map(self):
        device_map = self.__dict__.get("_map_obj")
        if device_map is None:
            loader = self.__dict__.get("_map_loader")
            if loader is None:
                raise AttributeError("_map")
            device_map = self.__dict__["_map_obj"] = loader()
            self.__dict__["_map_loader"] = None
        return device_map

    @_map.setter
    def _map(self, value):
        self.__dict__["_map_obj"] = value

    @property
    def resident(self):
        """Whether the grid is in HBM already (False: a lazily read file nobody has asked for yet)."""
        return self.__dict__.get("_map_obj") is not None

    # ref densityAnalysis.py:148 sets ``diffDensityCutoff = meanDensity + 3 * stdDensity`` when the Fo-Fc map is loaded; here
    # the attribute computes itself on first use unless somebody assigned it (the value is the same; a lazily read map is
    # not brought in just to have it)
    @property
    def diffDensityCutoff(self):
        value = self.__dict__.get("_diffDensityCutoff")
        if value is None:
            value = self.__dict__["_diffDensityCutoff"] = self.meanDensity + 3 * self.stdDensity
        return value

    @diffDensityCutoff.setter
    def diffDensityCutoff(self, value):
        self.__dict__["_diffDensityCutoff"] = value

    @property
    def density(self):
        """The float32 grid [section][row][column] on the host (ref ccp4.py:337); fetched from HBM when the map never had a
        host copy."""
        if self._density is None:
            self._density = self._map.download()
        return self._density

    @density.setter
    def density(self, value):
        self._density = value

    @property
    def densityArray(self):
        """ref ccp4.py:338: the flat view of ``density`` (or whatever was assigned to it)."""
        if self._densityArray is not None:
            return self._densityArray
        return self._flatOf.densityArray if self._flatOf is not None else self.density.reshape(-1)

    @densityArray.setter
    def densityArray(self, value):
        self._densityArray = value

    @property
    def numStoredVoxels(self):
        """``densityArray.size`` without touching the host copy."""
        if self._densityArray is not None:
            return self._densityArray.size
        if self._flatOf is not None:
            return self._flatOf.numStoredVoxels
        return self.header.ncrs[0] * self.header.ncrs[1] * self.header.ncrs[2]

    # -- whole-map reductions -------------------------------------------------------
    def _stats(self):
        if self._meanDensity is None:
            self._meanDensity, self._stdDensity = self._map.stats()

    @property
    def meanDensity(self):
        """ref ccp4.py:343-352 (np.mean of all stored voxels) -- fp64 device reduction."""
        self._stats()
        return self._meanDensity

    @property
    def stdDensity(self):
        """ref ccp4.py:354-363 (population std, two-pass)."""
        self._stats()
        return self._stdDensity

    def getTotalAbsDensity(self, densityCutoff):
        """ref ccp4.py:365-376 -> cutils.pyx:28-39 (strict |v| > float32(cutoff), cached per cutoff)."""
        if densityCutoff not in self._totalAbsDensity:
            self._totalAbsDensity[densityCutoff] = self._map.sum_of_abs(densityCutoff)
        return self._totalAbsDensity[densityCutoff]

    # -- point access ---------------------------------------------------------------
    def getPointDensityFromCrs(self, crsCoord):
        """ref ccp4.py:378-387 -> cutils.pyx:125-145 (periodic wrap contract)."""
        return float(self._map.point_density(np.asarray([list(crsCoord)], dtype=np.int32))[0])

    def getPointDensityFromXyz(self, xyzCoord):
        """ref ccp4.py:389-398."""
        return self.getPointDensityFromCrs(self.header.xyz2crsCoord(xyzCoord))

    # -- sphere gathers -------------------------------------------------------------
    @staticmethod
    def _is_single(xyzCoords):
        return isinstance(xyzCoords[0], (np.floating, float, int, np.integer))

    def _sphere(self, xyzCoords, radius, densityCutoff):
        xyz = np.asarray(xyzCoords, dtype=np.float64).reshape(-1, 3)
        if isinstance(radius, (list, tuple, np.ndarray)):
            radii = np.asarray(radius, dtype=np.float32)
        else:
            radii = np.full(len(xyz), radius, dtype=np.float32)
        return xyz, radii

    def getSphereCrsFromXyz(self, xyzCoord, radius, densityCutoff=0):
        """ref ccp4.py:400-416 -> cutils.pyx:220-248; returns a list of raw (c, r, s) lists."""
        xyz, radii = self._sphere([xyzCoord], radius, densityCutoff)
        bl = self._map.sphere_blobs(xyz, radii, np.array([0, 1], dtype=np.int64), densityCutoff)
        crs, _ = bl.voxels()
        return [list(map(int, v)) for v in crs]

    def getTotalDensityFromXyz(self, xyzCoord, radius, densityCutoff=0):
        """ref ccp4.py:418-435."""
        xyz, radii = self._sphere([xyzCoord], radius, densityCutoff)
        bl = self._map.sphere_blobs(xyz, radii, np.array([0, 1], dtype=np.int64), densityCutoff)
        return float(np.sum(bl.stats()["totalDensity"]))

    def findAberrantBlobs(self, xyzCoords, radius, densityCutoff=0):
        """ref ccp4.py:437-461: sphere (or sphere-union) voxels above the cutoff, clustered."""
        if self._is_single(xyzCoords):
            xyzCoords = [xyzCoords]
        xyz, radii = self._sphere(xyzCoords, radius, densityCutoff)
        bl = self._map.sphere_blobs(xyz, radii, np.array([0, len(xyz)], dtype=np.int64), densityCutoff)
        return DensityBlob.listFromDevice(bl, self)

    # -- radial profiles (no reference counterpart) ----------------------------------
    def radialProfiles(self, xyzCoordList, maxRadius, nShells=20, densityCutoff=0):
        """The density around every coordinate by distance, in ONE device call (``pdbeda_radial_profiles`` in include/pdbeda.h
        has the contract): the sphere of ``maxRadius`` around a coordinate -- the voxels of ``getSphereCrsFromXyz`` -- is cut into
        ``nShells`` concentric shells of equal width.  A dict of (n, nShells) arrays ``n`` / ``sum`` (voxels and density of a shell,
        no filter), ``nSig`` / ``sumSig`` (the voxels that pass ``densityCutoff``, strict, as ``getSphereCrsFromXyz``) and the (n,)
        flags ``valid``.  Coordinates do not see each other: spheres that overlap count the shared voxels once each."""
        xyz = np.asarray(xyzCoordList, dtype=np.float64).reshape(-1, 3)
        return self._map.radial_profiles(xyz, maxRadius, nShells, densityCutoff)

    # -- nearest-atom partition (no reference counterpart) -----------------------------
    def partition(self, xyzList, maxDistance, cutoff=0.0, owners=False):
        """Every voxel of the non-repeating box (the domain of ``createFullCrsList``) to the coordinate nearest to it within
        ``maxDistance`` -- ties to the lowest index -- or to nobody, each voxel counted ONCE, in one device call
        (``pdbeda_map_partition`` in include/pdbeda.h has the contract).  A dict of (n,) arrays ``n`` / ``sum`` (voxels owned and their
        density), ``nPos`` / ``sumPos`` (density > cutoff), ``nNeg`` / ``sumNeg`` (density < -cutoff; strict, cutoff >= 0), the totals
        over the unowned voxels ``unownedN`` (n, n_pos, n_neg) and ``unownedSum`` (sum, sum_pos, sum_neg, sum of squares) and, with
        ``owners``, ``owner``: an (ns', nr', nc') int32 array of the box, -1 where nobody owns the voxel."""
        xyz = np.asarray(xyzList, dtype=np.float64).reshape(-1, 3)
        return self._map.partition(xyz, maxDistance, cutoff, owners)

    # -- the map between voxels: trilinear density, Q-scores (no reference counterpart) --
    def getInterpolatedDensityFromXyz(self, xyzCoord):
        """The trilinear density at a coordinate (a float) or at a list of coordinates (an array), in one device call
        (``pdbeda_interp_density`` in include/pdbeda.h has the contract): the eight voxels around the point under the wrap rule of
        ``getPointDensityFromCrs``, 0 where nothing is stored.  On a voxel centre it IS ``getPointDensityFromXyz``."""
        single = self._is_single(xyzCoord)
        values, _ = self._map.interp_density(np.asarray([xyzCoord] if single else xyzCoord, dtype=np.float64).reshape(-1, 3))
        return float(values[0]) if single else values

    def qScores(self, xyzList, scored=None, sigma=0.6, step=0.1, nShells=21, nPoints=8):
        """Q-scores (Pintilie et al. 2020) of the coordinates ``scored`` (indices into ``xyzList``; None: all) among ALL of ``xyzList``,
        in one device call (``pdbeda_atom_qscores`` in include/pdbeda.h has the contract): the map sampled on ``nShells`` spheres of
        radius k * step around a coordinate, only where no other coordinate is nearer, correlated with exp(-r^2 / (2 sigma^2)).  The
        sample directions are the fixed lattices of ``qScoreTables`` (``nPoints`` on the coarsest, doubled until ``nPoints`` survive): the
        values are reproducible and are not MapQ's digit for digit.  A dict of ``q``, ``nPoints``, ``valid`` ((n,)), ``shellN`` /
        ``shellMean`` ((n, nShells)) and ``counters``."""
        levels = 1
        while levels < 4 and int(nPoints) * 2 ** levels <= 64:      # (a level is one wave pass: 64 candidates at the most)
            levels += 1
        ref, unit, offsets = qScoreTables(sigma, step, nShells, nPoints, levels)
        xyz = np.asarray(xyzList, dtype=np.float64).reshape(-1, 3)
        return self._map.qscores(xyz, scored, step, ref, unit, offsets, nPoints)

    # -- from the model to a map (no reference counterpart) ------------------------------
    def modelDensity(self, xyz, amp, expo, radii):
        """The calculated density of Gaussian atoms on THIS map's grid, as a device-made DensityMatrix (``pdbeda_model_density`` in
        include/pdbeda.h has the contract): atom a adds sum_j amp[a][j] exp(-expo[a][j] d^2) to every stored voxel within radii[a] of
        it.  ``amp`` / ``expo`` are (n,) or (n, n_terms <= 6) -- ``gaussianAtomTerms`` / ``modelRadii`` make the one-term model.
        Nothing wraps: pass the symmetry atoms.  This map's density is not read.  ``modelCounters`` of the result: the shift S of the
        integer sums, the most atoms a tile staged, the tiles that staged more than once."""
        device_map = type(self._map).model_density(self._map, xyz, amp, expo, radii)
        out = DensityMatrix.fromDeviceMap(self.header, self.origin, device_map, self.pdbid, self._ctx)
        out.modelCounters = device_map.model_counters
        return out

    def pairMoments(self, other, floor=None):
        """(n, Sa, Sb, Saa, Sbb, Sab) of this map (a) and ``other`` (b) over the voxels of the non-repeating box where both are finite
        and b > floor (strict; None keeps every finite pair), in one device call with a fixed summation order
        (``pdbeda_map_pair_moments``)."""
        n, sums = self._map.pair_moments(other._map, floor)
        return (n,) + tuple(float(v) for v in sums)

    def correlate(self, other, floor=None):
        """The correlation of this map with ``other`` over ``pairMoments``' voxels and the least-squares fit self ~ scale * other +
        offset: a dict ``n``, ``cc``, ``scale``, ``offset``.  cc is NaN where either variance is zero (or n == 0), scale and offset
        where ``other``'s is."""
        n, sa, sb, saa, sbb, sab = self.pairMoments(other, floor)
        nan = float("nan")
        if n == 0:
            return {"n": 0, "cc": nan, "scale": nan, "offset": nan}
        va, vb, cov = saa - sa * sa / n, sbb - sb * sb / n, sab - sa * sb / n
        scale = cov / vb if vb > 0 else nan
        return {"n": n, "cc": min(1.0, max(-1.0, cov / math.sqrt(va * vb))) if va > 0 and vb > 0 else nan, "scale": scale,
                "offset": (sa - scale * sb) / n if vb > 0 else nan}

    # -- from a map back to the atoms: gradient sums, real-space refinement (no reference counterpart) --
    def atomMoments(self, xyz, expo, radii, uniqueBox=False):
        """The adjoint of ``modelDensity`` with THIS map as the weight w, in one device call (``pdbeda_atom_moments`` in include/pdbeda.h
        has the contract): per atom and term the sums over the voxels within radii[a] -- ``modelDensity``'s pair set exactly -- of w e,
        w e dx, w e dy, w e dz and w e d^2 with e = exp(-expo d^2) and (dx, dy, dz) = voxel - atom.  Over all stored voxels, or with
        ``uniqueBox`` over the non-repeating box, the domain of ``pairMoments``.  A dict ``moments`` (n, terms, 5), ``nVoxels`` (n,) and
        ``counters`` (the shift S of the integer sums, the voxels of the largest box, the atoms whose box the domain clipped).  Results
        are the same bits in every run and for every order of the atoms.  ``gaussianAtomGradients`` turns them into derivatives."""
        return self._map.atom_moments(xyz, expo, radii, uniqueBox)

    # -- what fits in a blob: rigid-fragment pose search (no reference counterpart) --
    def poseScores(self, fragXyz, weights, rotations, centres, topK=1, floor=-np.inf, maxLow=None, allowOutside=False, full=False):
        """Every pose (centre, rotation) of a rigid fragment scored on THIS map in one device call (``pdbeda_pose_scores`` in include/pdbeda.h
        has the contract).  ``fragXyz`` (n, 3) is relative to the pivot (``fragmentFrame``), ``rotations`` (n_rot, 3, 3) come from
        ``rotationLattice`` / ``rotationsNear``.  The score of a pose is sum_a weights[a] * (the trilinear density at atom a); a pose is rejected
        when more than ``maxLow`` atoms read less than ``floor`` (None: no limit), when its score is NaN, or -- unless ``allowOutside`` -- when
        an atom reads a voxel that is not stored.  A dict ``bestRot`` / ``bestScore`` / ``bestLow`` ((n_centres, topK): a centre's kept poses,
        best first; ties go to the lower rotation index; -1 / 0.0 / 0 beyond them), ``nKept`` (n_centres,), with ``full`` also ``scores`` /
        ``low`` / ``kept`` ((n_centres, n_rot)), and ``counters`` (centres that read the map directly, the largest staged box, rejected
        poses).  The same bits in every run; permuting the centres permutes the rows."""
        w = np.ones(len(np.asarray(fragXyz).reshape(-1, 3))) if weights is None else weights
        return self._map.pose_scores(fragXyz, w, rotations, centres, topK, floor, maxLow, allowOutside, full)

    def searchFragment(self, fragXyz, weights, centres, rotations=None, nRotations=4096, nBest=3, levels=4, nNear=256, nCloud=27, angle=None,
                       floor=-np.inf, maxLow=None, allowOutside=False):
        """Coarse-to-fine pose search with ``poseScores``, every level ONE device call.  Level 0 scores ``rotations`` (default
        ``rotationLattice(nRotations)``) at every centre and keeps the ``nBest`` best poses over all centres.  Each later level, for every pose
        kept so far, scores ``rotationsNear(R, angle_l, nNear)`` (the pose's own rotation first) at a cloud of ``nCloud`` centres -- the pose's
        own centre first, then a cubic lattice of half-width step_l around it; the levels' calls are batched into one by listing all
        clouds' centres against all poses' rotations and reading each pose's own block.  angle_l and step_l halve from level to level, starting at
        ``angle`` (default: the lattice's spacing, (16 pi^2 / n_rot)^(1/3), capped at pi) and half a grid step.  A refined pose replaces
        its parent only if its score is NOT lower.  It stops after ``levels`` levels.  Returns a list of dicts, best first: ``centre``, ``rotation``,
        ``score``, ``low``, ``xyz`` (the placed atoms, ``placeFragment``) and ``trace`` (the score after every level, level 0 first)."""
        frag = np.asarray(fragXyz, dtype=np.float64).reshape(-1, 3)
        w = np.ones(len(frag)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        rot = rotationLattice(nRotations) if rotations is None else np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)
        rule = dict(floor=floor, maxLow=maxLow, allowOutside=allowOutside)
        first = self.poseScores(frag, w, rot, centres, topK=min(int(nBest), _native.POSE_MAX_TOP), **rule)
        rows = [(float(first["bestScore"][c, k]), c, k) for c in range(len(centres)) for k in range(first["bestRot"].shape[1]) if first["bestRot"][c, k] >= 0]
        rows.sort(key=lambda r: (-r[0], r[1], r[2]))
        poses = [{"centre": centres[c].copy(), "rotation": rot[first["bestRot"][c, k]].copy(), "score": s, "low": int(first["bestLow"][c, k]), "trace": [s]}
                 for s, c, k in rows[:int(nBest)]]
        theta = min(np.pi, (16.0 * np.pi ** 2 / max(len(rot), 1)) ** (1.0 / 3.0)) if angle is None else float(angle)
        step = 0.5 * float(min(self.header.gridLength))
        side = max(1, int(round(int(nCloud) ** (1.0 / 3.0))))
        ticks = (np.arange(side, dtype=np.float64) - 0.5 * (side - 1)) / max(0.5 * (side - 1), 1.0)
        cloud = np.array([[a, b, c] for a in ticks for b in ticks for c in ticks if (a, b, c) != (0.0, 0.0, 0.0)], dtype=np.float64).reshape(-1, 3)
        for _ in range(int(levels)):
            if not poses:
                break
            near = [rotationsNear(p["rotation"], theta, nNear) for p in poses]
            around = [np.concatenate([p["centre"][None, :], p["centre"] + step * cloud]) for p in poses]
            m, per = len(near[0]), len(around[0])
            got = self.poseScores(frag, w, np.concatenate(near), np.concatenate(around), full=True, **rule)
            for j, p in enumerate(poses):      # pose j's own block of the table: its centres against its rotations
                block = np.where(got["kept"][j * per:(j + 1) * per, j * m:(j + 1) * m], got["scores"][j * per:(j + 1) * per, j * m:(j + 1) * m], -np.inf)
                c, r = np.unravel_index(int(np.argmax(block)), block.shape)      # (the first maximum: the pose itself on a tie)
                if block[c, r] >= p["score"] and block[c, r] > -np.inf:
                    p["centre"], p["rotation"], p["score"] = around[j][c].copy(), near[j][r].copy(), float(block[c, r])
                    p["low"] = int(got["low"][j * per + c, j * m + r])
                p["trace"].append(p["score"])
            theta, step = 0.5 * theta, 0.5 * step
        poses.sort(key=lambda p: -p["score"])
        for p in poses:
            p["xyz"] = placeFragment(frag, p["centre"], p["rotation"])
        return poses

    def _leastSquaresTarget(self, model):
        """(T, scale, offset, cc) of this map against ``model`` over the non-repeating box: T = sum (self - scale model - offset)^2 / 2 at
        the least-squares scale and offset, from the device's ``pairMoments``."""
        n, sa, sb, saa, sbb, sab = self.pairMoments(model)
        if n == 0:
            raise RuntimeError("no finite voxel pair in the non-repeating box")
        va, vb, cov = saa - sa * sa / n, sbb - sb * sb / n, sab - sa * sb / n
        if not vb > 0:
            raise RuntimeError("the model density is constant over the map: there is no scale to fit")
        scale = cov / vb
        return 0.5 * max(va - cov * cov / vb, 0.0), scale, (sa - scale * sb) / n, (cov / math.sqrt(va * vb) if va > 0 else float("nan"))

    def _residual(self, model, scale, offset):
        """self - scale * model - offset as a resident map: two ``pdbeda_map_combine`` calls, the second against a map of ones."""
        if self.__dict__.get("_ones") is None:
            nc, nr, ns = (int(v) for v in self.header.ncrs)
            self.__dict__["_ones"] = _native.DeviceMap(self._ctx, np.ones((ns, nr, nc), dtype=np.float32), self.header.geometry())
        kind = type(self._map)
        return self._made(kind.combine(kind.combine(self._map, model._map, -scale), self.__dict__["_ones"], -offset))

    def refineGaussianAtoms(self, xyz, electrons, bfactors, occupancies, what=("xyz", "b"), cycles=10, maxShift=0.3, images=None, imageAtoms=None,
                            blur=0.0, minB=MODEL_MIN_B, nSigma=MODEL_N_SIGMA, maxHalvings=6):
        """Real-space refinement of one-Gaussian atoms (``gaussianAtomTerms``) against THIS map, on plain arrays; no voxel leaves the device.
        A cycle: ``modelDensity`` of the atoms; ``pairMoments`` for the scale s and offset o of self ~ s calc + o; the residual R = self -
        s calc - o by ``pdbeda_map_combine``; ``atomMoments(uniqueBox=True)`` of R; a host step.  The target is T = sum (self - s calc -
        o)^2 / 2 over the non-repeating box.  Because s and o MINIMISE T, its derivatives with respect to them vanish, and dT/dtheta =
        -s sum_v R d rho / d theta at fixed s and o is the FULL derivative of the profiled target (the envelope argument).  The step is
        damped diagonal Gauss-Newton, the curvature from the closed-form integrals of an isolated Gaussian (``gaussianAtomCurvatures``):
        shifts are capped at ``maxShift`` A, B stays >= ``minB``, occupancy in [0, 1].  A step is taken only if T, evaluated on the
        device, goes down; otherwise it is halved, ``maxHalvings`` times at the most, and a cycle without an accepted step ends the loop.
        ``what``: any of "xyz", "b", "occ".  ``images``: operators (3 x 4) whose copies of every atom make the model (the identity is not
        implied: list it); ``imageAtoms`` = (rows, operators) names the copies one by one instead (copy k is atom rows[k] under
        operators[k]).  The gradient of a copy comes back through the transpose of its rotation.  Returns a dict ``xyz``, ``bfactors``,
        ``occupancies`` and ``trace``: lists ``T``, ``scale``, ``cc`` (before the first cycle and after every cycle run) and ``halvings``
        (per cycle; -1: no step was accepted)."""
        xyz = np.array(xyz, dtype=np.float64).reshape(-1, 3)
        n = len(xyz)
        z = np.asarray(electrons, dtype=np.float64).reshape(-1)
        b = np.array(bfactors, dtype=np.float64).reshape(-1)
        occ = np.array(occupancies, dtype=np.float64).reshape(-1)
        unknown = set(what) - {"xyz", "b", "occ"}
        if unknown:
            raise ValueError("what: unknown parameter kinds %s" % sorted(unknown))
        if imageAtoms is not None:
            rows = np.asarray(imageAtoms[0], dtype=np.int64).reshape(-1)
            ops = np.asarray(imageAtoms[1], dtype=np.float64).reshape(-1, 3, 4)
        else:
            each = [identityOperator()] if images is None else [_operator(op) for op in images]
            rows = np.tile(np.arange(n, dtype=np.int64), len(each))
            ops = np.repeat(np.array(each, dtype=np.float64).reshape(-1, 3, 4), n, axis=0)
        copies = np.bincount(rows, minlength=n).astype(np.float64)
        unitVolume = float(self.header.unitVolume)

        def place(xyz, b, occ):
            where = np.einsum("kij,kj->ki", ops[:, :, :3], xyz[rows]) + ops[:, :, 3]
            amp, expo, bEff = gaussianAtomTerms(z[rows], b[rows], occ[rows], blur=blur, minB=minB)
            radii = modelRadii(bEff, nSigma)
            return where, expo, radii, self.modelDensity(where, amp, expo, radii)

        where, expo, radii, model = place(xyz, b, occ)
        target, scale, offset, cc = self._leastSquaresTarget(model)
        trace = {"T": [target], "scale": [scale], "cc": [cc], "halvings": []}
        for _ in range(int(cycles)):
            moments = self._residual(model, scale, offset).atomMoments(where, expo, radii, uniqueBox=True)["moments"]
            grad = foldImageGradients(gaussianAtomGradients(moments, z[rows], b[rows], occ[rows], blur=blur, minB=minB), rows, ops[:, :, :3], n)
            gradT = {k: -scale * v for k, v in grad.items()}
            curv = gaussianAtomCurvatures(z, b, occ, unitVolume, blur=blur, minB=minB)
            step = gaussNewtonStep(gradT, {k: v * copies for k, v in curv.items()}, scale, what, maxShift)
            taken = -1
            for h in range(int(maxHalvings) + 1):
                f = 0.5 ** h
                xyz2 = xyz + f * step["xyz"]
                b2 = np.maximum(b + f * step["b"], float(minB)) if "b" in what else b
                occ2 = np.clip(occ + f * step["occ"], 0.0, 1.0) if "occ" in what else occ
                trial = place(xyz2, b2, occ2)
                t2, s2, o2, cc2 = self._leastSquaresTarget(trial[3])
                if t2 < target:
                    xyz, b, occ, taken = xyz2, b2, occ2, h
                    where, expo, radii, model = trial
                    target, scale, offset, cc = t2, s2, o2, cc2
                    break
            trace["halvings"].append(taken)
            trace["T"].append(target); trace["scale"].append(scale); trace["cc"].append(cc)
            if taken < 0:
                break
        return {"xyz": xyz, "bfactors": b, "occupancies": occ, "trace": trace}

    # -- from a map to a map through a neighbourhood (no reference counterpart) ------------
    def _made(self, device_map):
        return DensityMatrix.fromDeviceMap(self.header, self.origin, device_map, self.pdbid, self._ctx)

    def filtered(self, tapsC, tapsR, tapsS, renormalize=False):
        """This map filtered along its column, row and section axes with the given taps (odd lengths, correlation form), as a device-made
        DensityMatrix (``pdbeda_map_filter`` in include/pdbeda.h has the contract): the faces follow the map's own wrap rule -- a full
        cell is periodic, a cut-out sees zeros --, and ``renormalize`` divides by the weight of the taps that met stored voxels (taps >= 0),
        which keeps a weighted mean a mean at the faces of a cut-out."""
        return self._made(self._map.filter(tapsC, tapsR, tapsS, renormalize))

    def _gaussianTapsPerAxis(self, sigma, truncate, voxels):
        """gaussianTaps for the three crs axes: ``sigma`` in grid steps (``voxels``) or in Angstrom over gridLength (orthogonal cells only)."""
        if voxels:
            sigmas = [float(sigma)] * 3
        else:
            if not self.header.orthogonal:
                raise ValueError("a separable filter along the grid axes of a skewed cell is not isotropic: pass sigma in grid steps with voxels=True")
            sigmas = [float(sigma) / self.header.gridLength[self.header.map2crs[k]] for k in range(3)]
        taps = [gaussianTaps(s, truncate) for s in sigmas]
        for axis, t in zip("crs", taps):
            if len(t) // 2 > FILTER_MAX_RADIUS:
                raise ValueError("a Gaussian of sigma %g reaches radius %d along %s, beyond the filter's largest radius %d" % (sigma, len(t) // 2, axis, FILTER_MAX_RADIUS))
        return taps

    def gaussianFilter(self, sigma, truncate=4.0, voxels=False, renormalize=True):
        """This map smoothed by a Gaussian of ``sigma`` Angstrom (``voxels=True``: grid steps), cut off at ``truncate`` sigmas, as a
        device-made DensityMatrix.  Angstrom are turned into grid steps per crs axis from ``gridLength``, on orthogonal cells only: a skewed
        cell raises ValueError unless ``voxels=True``; so does a radius beyond PDBEDA_FILTER_MAX_RADIUS."""
        taps = self._gaussianTapsPerAxis(sigma, truncate, voxels)
        return self.filtered(taps[0], taps[1], taps[2], renormalize)

    def localStats(self, other=None, taps=None, sigma=None, truncate=4.0, voxels=False, stdFloor=0.0):
        """Windowed statistics of this map (``pdbeda_map_local_stats``): a dict of device-made DensityMatrix objects ``mean``, ``std`` and
        ``z`` (the voxel's distance from its local mean in local standard deviations, never below ``stdFloor``), and with ``other`` also
        ``meanOther``, ``stdOther`` and ``cc``, the local correlation of the two maps.  The window is ``taps`` (one array for all axes, or three,
        all >= 0) or a Gaussian of ``sigma`` as in ``gaussianFilter``.  Cells the window finds nothing for are 0, never NaN."""
        if (taps is None) == (sigma is None):
            raise ValueError("localStats takes either taps or sigma")
        if taps is None:
            taps = self._gaussianTapsPerAxis(sigma, truncate, voxels)
        elif np.ndim(taps[0]) == 0:
            taps = [taps, taps, taps]
        made = self._map.local_stats(None if other is None else other._map, taps[0], taps[1], taps[2], stdFloor)
        names = {"mean_a": "mean", "std_a": "std", "z_a": "z", "mean_b": "meanOther", "std_b": "stdOther", "cc": "cc"}
        return dict((names[key], self._made(device_map)) for key, device_map in made.items())

    # -- from a region of a map to a map: the ordered spread of a mask (no reference counterpart) ------------------------
    def spread(self, offsets, values, threshold=0.5, below=False, base=None, counters=False):
        """The raw call (``pdbeda_map_spread`` in include/pdbeda.h has the contract), as a device-made DensityMatrix: every stored voxel gets
        ``values[t]``, t the first entry of the ordered ``offsets`` table (n x 3 int32: dc, dr, ds) that leads from it to a seed -- a voxel
        > ``threshold``, or < it with ``below`` -- under the map's own wrap rule, and ``values[n]`` where none does.  With ``base`` (a
        DensityMatrix on this grid) the voxel is base * value, rounded once.  With ``counters`` the result is (map, {"seeds", "reached",
        "rows"}): the seeds among the stored voxels, the voxels with a seed in reach, 1 if the table was searched row by row."""
        made = self._map.spread(offsets, values, threshold, below, None if base is None else base._map, counters)
        return (self._made(made[0]), made[1]) if counters else self._made(made)

    def dilated(self, radius, threshold=0.5):
        """1.0 within ``radius`` Angstrom of a voxel > ``threshold``, 0.0 elsewhere."""
        offsets = spreadTable(self.header, radius)[0]
        return self.spread(offsets, np.append(np.ones(len(offsets), dtype=np.float32), np.float32(0.0)), threshold)

    def eroded(self, radius, threshold=0.5):
        """The complement of the dilated complement: 0.0 within ``radius`` Angstrom of a voxel < ``threshold``, 1.0 elsewhere.  What lies outside
        a cut-out is no background: its faces are not eroded.  (A voxel that EQUALS the threshold is neither mask nor background.)"""
        offsets = spreadTable(self.header, radius)[0]
        return self.spread(offsets, np.append(np.zeros(len(offsets), dtype=np.float32), np.float32(1.0)), threshold, below=True)

    def opened(self, radius, threshold=0.5):
        """Erosion, then dilation: what a ball of ``radius`` fits into."""
        return self.eroded(radius, threshold).dilated(radius)

    def closed(self, radius, threshold=0.5):
        """Dilation, then erosion: gaps a ball of ``radius`` does not fit into are filled."""
        return self.dilated(radius, threshold).eroded(radius)

    def distanceFrom(self, maxDistance, threshold=0.5, below=False, beyond=np.inf):
        """The distance in Angstrom (float32) from every voxel to the nearest seed within ``maxDistance``: the table's own distances, 0 on a
        seed, ``beyond`` where none is in reach."""
        offsets, distance = spreadTable(self.header, maxDistance)
        return self.spread(offsets, np.append(distance.astype(np.float32), np.float32(beyond)), threshold, below)

    def softMask(self, radius, width, threshold=0.5):
        """1 within ``radius`` Angstrom of a voxel > ``threshold``, a raised cosine down to 0 at ``radius + width`` (``softEdgeValues``)."""
        offsets, distance = spreadTable(self.header, float(radius) + float(width))
        return self.spread(offsets, softEdgeValues(distance, radius, width), threshold)

    def maskedBy(self, seeds, radius=0.0, width=0.0, threshold=0.5):
        """This map times the soft mask of ``seeds`` (a DensityMatrix on this grid), in ONE device call: ``seeds.softMask`` with this map as
        the call's ``base``."""
        offsets, distance = spreadTable(self.header, float(radius) + float(width))
        return seeds.spread(offsets, softEdgeValues(distance, radius, width), threshold, base=self)

    def atomMask(self, xyz, radii):
        """1.0 on every stored voxel within ``radii[a]`` of an atom ``xyz[a]``, else 0.0: ``modelDensity`` with one term of amplitude 1 and exponent
        0 counts the spheres that cover a voxel (exactly: the sums are integers), and the single offset (0, 0, 0) at threshold 0.5 turns the
        count into a mask.  Nothing wraps: pass the symmetry atoms."""
        n = len(np.asarray(xyz).reshape(-1, 3))
        count = self.modelDensity(xyz, np.ones(n), np.zeros(n), radii)
        return count.spread(np.zeros((1, 3), dtype=np.int32), np.array([1.0, 0.0], dtype=np.float32), 0.5)

    def solventMask(self, xyz, radii, probe=1.11, shrink=0.9):
        """1.0 in the solvent, 0.0 in the molecule (the flat bulk-solvent model's mask): the atoms grown by ``probe``, complemented, and what is
        left of the molecule shrunk back by a ball of ``shrink`` -- a voxel is solvent iff an uncovered voxel lies within ``shrink`` of it."""
        grown = self.atomMask(xyz, np.asarray(radii, dtype=np.float64) + float(probe))
        offsets = spreadTable(self.header, shrink)[0]
        return grown.spread(offsets, np.append(np.ones(len(offsets), dtype=np.float32), np.float32(0.0)), 0.5, below=True)

    def maskStats(self, mask, threshold=0.5):
        """(n, mean, standard deviation) of this map over the voxels of the non-repeating box where ``mask`` > ``threshold`` (``pairMoments``);
        NaN without a voxel."""
        n, sa, _, saa, _, _ = self.pairMoments(mask, threshold)
        if n == 0:
            return 0, float("nan"), float("nan")
        mean = sa / n
        return n, mean, math.sqrt(max(saa / n - mean * mean, 0.0))

    # -- from a map to a map on ANOTHER grid: resampling under coordinate operators (no reference counterpart) --------
    def resampled(self, header, ops=None, order=1, mean=False, fill=0.0, base=None, alpha=1.0, coverage=False):
        """This map on the grid of ``header`` (a DensityHeader: another entry's, ``cellHeader`` / ``boxHeader``), as a device-made
        DensityMatrix (``pdbeda_map_resample`` in include/pdbeda.h has the contract): every voxel of the destination is carried by the
        operators ``ops`` ([R | t] rows from DESTINATION to SOURCE coordinates; None: the identity) into this map and read there at ``order``
        0 (nearest), 1 (trilinear) or 3 (Catmull-Rom).  The first operator that finds stored voxels gives the value, or with ``mean`` all
        that do are averaged; ``fill`` where none does.  With ``base`` (a DensityMatrix on ``header``) the result is base + alpha * value.
        ``coverage=True`` returns (map, map of the number of operators that served each voxel).  ``resampleCounters`` of the result:
        covered and uncovered voxels, (tile, operator) pairs read from staged boxes and directly."""
        ops = identityOperator().reshape(1, 12) if ops is None else np.asarray(ops, dtype=np.float64).reshape(-1, 12)
        made, cover = self._map.resample(header.geometry(), ops, order, mean, fill, None if base is None else base._map, alpha, coverage)
        out = DensityMatrix.fromDeviceMap(header, header.origin, made, self.pdbid, self._ctx)
        out.resampleCounters = made.resample_counters
        return (out, DensityMatrix.fromDeviceMap(header, header.origin, cover, self.pdbid, self._ctx)) if coverage else out

    def symmetryExpanded(self, rotationMats, header=None, order=1):
        """This map under the space group's operators ``rotationMats`` (``PDBHeader.rotationMats``) on ``header`` (default: the whole unit
        cell, ``cellHeader(self.header)``): the identity first, then the operators as given, the first that reaches stored density
        serves a voxel; 0 where none does.  A symmetry operator is an isometry of the crystal, so pulling back through every one of them
        finds each copy."""
        ops = [identityOperator()] + [_operator(m) for m in rotationMats]
        return self.resampled(cellHeader(self.header) if header is None else header, np.array(ops).reshape(-1, 12), order=order)

    # -- reciprocal space (no reference counterpart) ---------------------------------------------------------------
    def fourier(self):
        """The 3-D Fourier transform of this map as a device-resident DensitySpectrum (``pdbeda_map_fft`` in include/pdbeda.h has the
        contract): numpy's ``rfftn`` of the stored box, which is the period.  Every axis must be a plannable length (``isFourierSize``):
        transform a whole cell (``symmetryExpanded``, on ``fourierHeader`` where the sampling is not plannable) or a ``fourierBox``."""
        return DensitySpectrum(self, self._map.fft())

    def fourierFiltered(self, table, s2Max, beyond=0.0):
        """This map with every Fourier coefficient multiplied by the radial table g(s^2) (``DensitySpectrum.scaled``), as a device-made
        DensityMatrix: transform, scale, inverse transform, nothing leaves the device."""
        spec = self.fourier()
        spec.scale(table, s2Max, beyond)
        return spec.toMap()

    def resolutionCut(self, dMin, dMax=None, softness=0.1):
        """This map cut at ``dMin`` Angstrom (and, with ``dMax``, without the terms below 1 / dMax): ``resolutionTable``'s raised-cosine window."""
        table = resolutionTable(dMin, dMax, softness)
        s2max = ((1.0 + 0.5 * float(softness)) / float(dMin)) ** 2 * (1.0 + 2.0 ** -20)
        return self.fourierFiltered(table, s2max, 0.0)

    def sharpened(self, B):
        """This map with every coefficient multiplied by exp(-B s^2 / 4): B < 0 sharpens, B > 0 blurs (an isotropic B-factor)."""
        s2max = maxS2(self.header)
        return self.fourierFiltered(bFactorTable(B, s2max), s2max, 0.0)

    def shellStats(self, other=None, nShells=20, dMin=None, dMax=None):
        """``DensitySpectrum.shells`` of this map's transform (against ``other``'s, a DensityMatrix of the same shape)."""
        return self.fourier().shells(None if other is None else other.fourier(), edges=shellEdges(self.header, nShells, dMin, dMax))

    def fsc(self, other, nShells=20, dMin=None, dMax=None):
        """The Fourier shell correlation of this map with ``other``: a dict ``d_max``, ``d_min``, ``n``, ``fsc`` per resolution shell."""
        table = self.shellStats(other, nShells, dMin, dMax)
        return dict((key, table[key]) for key in ("d_max", "d_min", "n", "fsc"))

    def structureFactors(self, hkl):
        """Structure factors of a WHOLE-CELL map at the Miller indices ``hkl`` ((n, 3), on the cell axes a*, b*, c*) in the crystallographic
        convention F(h) = V / N sum rho(x) exp(+2 pi i h.x), x the fractional coordinate of a voxel, crsStart included: complex128 (n,).
        Any integer index is taken modulo the sampling.  ValueError for a map that does not store exactly one cell."""
        h = self.header
        if [int(v) for v in h.ncrs] != [int(v) for v in h.crsInterval]:
            raise ValueError("structureFactors takes a map of the whole unit cell (symmetryExpanded on cellHeader / fourierHeader)")
        hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
        idx = np.stack([hkl[:, h.map2crs[k]] for k in range(3)], axis=1)
        if len(idx) and np.abs(idx).max() >= 2 ** 31:
            raise ValueError("structureFactors: an index beyond int32")
        raw = self.fourier().at(idx)
        turn = sum(idx[:, k] * int(h.crsStart[k]) / float(h.crsInterval[k]) for k in range(3)) if len(idx) else np.zeros(0)
        volume = float(h.unitVolume) * float(h.xyzInterval[0]) * float(h.xyzInterval[1]) * float(h.xyzInterval[2])
        return (volume / float(h.ncrs[0] * h.ncrs[1] * h.ncrs[2])) * np.conj(raw) * np.exp(2j * np.pi * np.asarray(turn, dtype=np.float64))

    def fourierBox(self, margin=0.0):
        """This map (a cut-out) embedded in zeros on a plannable box, as a device-made DensityMatrix: the same cell and sampling, ``margin``
        Angstrom (in grid steps of each axis, rounded up) added on every side and every axis then grown at its high end to the next
        plannable length; ``resampled`` at order 0 with the identity operator and fill 0.  Where the grown box leaves the cell it reads the
        cell's periodic copies, as every call does."""
        h = self.header
        pad = [int(math.ceil(float(margin) / h.gridLength[h.map2crs[k]] - 1e-9)) for k in range(3)]
        if min(pad) < 0:
            raise ValueError("fourierBox: margin >= 0")
        ncrs = [fourierSize(int(h.ncrs[k]) + 2 * pad[k]) for k in range(3)]
        start = [int(h.crsStart[k]) - pad[k] for k in range(3)]
        box = _headerFromFields(ncrs, start, h.xyzInterval, h.xyzLength, (h.alpha, h.beta, h.gamma), (h.col2xyz, h.row2xyz, h.sec2xyz), h.spaceGroup)
        return self.resampled(box, order=0, fill=0.0)

    # -- whole-map blobs ------------------------------------------------------------
    def createFullBlobList(self, cutoff):
        """ref ccp4.py:463-473: threshold the non-repeating box and cluster (None for cutoff == 0)."""
        if np.float32(cutoff) == 0:
            return None
        return DensityBlob.listFromDevice(self._map.full_blobs(cutoff), self, wholeMap=True)

    def createFullBlobLists(self, cutoff):
        """Fused green (+cutoff) and red (-cutoff) lists from ONE pass over the grid."""
        green, red = self._map.full_blobs_pm(abs(cutoff), -abs(cutoff))
        return DensityBlob.listFromDevice(green, self, wholeMap=True), DensityBlob.listFromDevice(red, self, wholeMap=True)

    def createBlobList(self, crsList):
        """ref ccp4.py:475-485: cluster an explicit (raw) crs list into blobs."""
        crs = np.asarray([list(c) for c in crsList], dtype=np.int32).reshape(-1, 3)
        return DensityBlob.listFromDevice(self._map.list_blobs(crs), self)

    # -- peaks (no reference counterpart) -------------------------------------------
    @staticmethod
    def _deviceListOf(blobList):
        """The device list behind what ``createFullBlobList`` returned (None stays None)."""
        if blobList is None:
            return None
        if not isinstance(blobList, DeviceBlobs) or len(blobList._segments) != 1:
            raise ValueError("blobList must be what createFullBlobList / createFullBlobLists returned")
        return blobList._segments[0].bl

    def findPeaks(self, cutoff, blobList=None):
        """The local maxima with density >= cutoff (minima with density <= cutoff when it is negative) of the non-repeating box,
        strongest first, as ``DensityPeak`` items (``pdbeda_map_peaks`` in include/pdbeda.h has the contract); None for cutoff == 0,
        as ``createFullBlobList``.  blobList: ``createFullBlobList(cutoff)`` of this map -- every peak then knows its blob."""
        if np.float32(cutoff) == 0:
            return None
        return DevicePeaks(self._map.peaks(cutoff, self._deviceListOf(blobList)), self, cutoff, blobList)

    def findPeakLists(self, cutoff, blobLists=None):
        """Fused (positive, negative) peak lists at +-|cutoff| from ONE pass over the grid; blobLists: the pair
        ``createFullBlobLists(cutoff)`` returned, or None."""
        green, red = blobLists if blobLists is not None else (None, None)
        pos, neg = self._map.peaks_pm(abs(cutoff), -abs(cutoff), self._deviceListOf(green), self._deviceListOf(red))
        return DevicePeaks(pos, self, abs(cutoff), green), DevicePeaks(neg, self, -abs(cutoff), red)


class DensityPeak(object):
    """One local extremum of a map: ``crs`` (raw voxel), ``height`` (the voxel's value), ``xyz`` / ``refinedHeight`` (vertex of
    one parabola per axis), ``blobIndex`` (in the blob list the search was given, else -1), ``onBorder`` (a voxel on the edge of
    the stored box: the extremum may be the edge's).  A peak of a device list also has the ``BASIN_COLUMNS`` of its basin as read-only
    attributes, made for the whole list on first use (``basinFinish``)."""
    __slots__ = ("crs", "height", "xyz", "refinedHeight", "blobIndex", "onBorder", "densityMatrix", "_peaks", "_index")

    def __init__(self, crs, height, xyz, refinedHeight, blobIndex, onBorder, densityMatrix=None):
        self.crs, self.height, self.xyz, self.refinedHeight = crs, height, xyz, refinedHeight
        self.blobIndex, self.onBorder, self.densityMatrix = blobIndex, onBorder, densityMatrix

    def __repr__(self):
        return "DensityPeak(crs=%r, height=%r)" % (self.crs, self.height)

    def _basinValue(self, name):
        peaks = getattr(self, "_peaks", None)
        if peaks is None:
            raise AttributeError("%s is known only for a peak that comes from a device list (findPeaks, findPeakLists)" % name)
        value = peaks.basinColumns()[name][self._index]
        return value.tolist() if isinstance(value, np.ndarray) else value.item()


class DevicePeaks(collections.abc.Sequence):
    """What ``findPeaks`` returns: a read-only sequence of ``DensityPeak`` in list order, lazy like ``DeviceBlobs`` -- the
    columns come from the device on first use, the objects are made when somebody reads one."""

    def __init__(self, pl, densityMatrix, cutoff=None, blobList=None):
        self._pl, self.densityMatrix = pl, densityMatrix
        self.cutoff, self.blobList = cutoff, blobList      # the float32 of ``cutoff`` is the job's; blobList: what the search was given, or None
        self._items = None
        self._basins = None

    def __len__(self):
        return len(self._pl)

    def columns(self):
        """{"crs", "height", "xyz", "refinedHeight", "blobIndex", "onBorder"} of all peaks as arrays."""
        rows = self._pl.rows()
        return {"crs": rows["crs"], "height": rows["height"], "xyz": rows["xyz"], "refinedHeight": rows["refinedHeight"],
                "blobIndex": rows["blob"], "onBorder": rows["onBorder"]}

    def counters(self):
        return self._pl.counters()

    def basinColumns(self):
        """``basinFinish`` of the list's basins (``pdbeda_peaklist_basins``): one row per peak, plus ``counters``.  Made on first use."""
        if self._basins is None:
            raw = self._pl.basins()
            cutoff = float(np.float32(self.cutoff)) if self.cutoff is not None else 0.0
            self._basins = basinFinish(self.densityMatrix.header, self.columns(), raw, cutoff)
            self._basins["counters"] = raw["counters"]
        return self._basins

    def basinVolume(self):
        """int32 [s][r][c] over the non-repeating box: the list index of every significant voxel's basin, -1 elsewhere (and for orphans)."""
        return self._pl.basins(volume=True)["basin"]

    def _all(self):
        if self._items is None:
            st = self.columns()
            self._items = [DensityPeak(*row, densityMatrix=self.densityMatrix)
                           for row in zip(st["crs"].tolist(), st["height"].tolist(), st["xyz"].tolist(), st["refinedHeight"].tolist(),
                                          st["blobIndex"].tolist(), st["onBorder"].tolist())]
            for index, peak in enumerate(self._items):
                peak._peaks, peak._index = self, index
        return self._items

    def __getitem__(self, i):
        return self._all()[i]

    def __iter__(self):
        return iter(self._all())

    def __repr__(self):
        return "DevicePeaks(%d peaks)" % len(self)


BASIN_COLUMNS = ("numVoxels", "totalDensity", "volume", "coordCenter", "centroid", "saddle", "prominence", "neighbour")


def basinFinish(header, peakColumns, raw, cutoff):
    """The basin columns of a peak list from the integer / fixed-point sums of ``pdbeda_peaklist_basins`` (``PeakList.basins()``) and the
    peaks' own columns -- a few vectorised fp64 operations per row, no voxel is touched.  A dict of arrays, one row per peak:

    ``numVoxels``, ``totalDensity``, ``volume`` (unitVolume x voxels), ``coordCenter`` (xyz of peak crs + s1 / n), ``centroid`` (xyz of
    peak crs + sw1 / |sum|: the density-weighted centre, sum rho xyz / sum rho, because ``crs2xyz`` is affine; the peak's own position
    where |sum| is 0), ``saddle`` (the highest pass to an adjacent basin, a map value; ``cutoff`` for a basin that is its whole blob),
    ``prominence`` (|height| - |saddle| in fp64 from the float32 values) and ``neighbour`` (the basin beyond the pass, -1 without one)."""
    n = np.asarray(raw["n"], dtype=np.int64)
    count = len(n)
    crs = np.asarray(peakColumns["crs"], dtype=np.float64).reshape(count, 3)
    total = np.asarray(raw["sum"], dtype=np.float64)
    s1 = np.asarray(raw["s1"], dtype=np.float64).reshape(count, 3)
    sw1 = np.asarray(raw["sw1"], dtype=np.float64).reshape(count, 3)
    weight = np.abs(total)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(weight[:, None] > 0, sw1 / weight[:, None], 0.0)
    neighbour = np.asarray(raw["neighbour"], dtype=np.int32)
    saddle = np.where(neighbour < 0, np.float32(cutoff), np.asarray(raw["saddle"], dtype=np.float32)).astype(np.float32)
    height = np.asarray(peakColumns["height"], dtype=np.float32)
    xyz = lambda at: header.crs2xyz_array(at).reshape(count, 3) if count else np.zeros((0, 3))
    return {"numVoxels": n, "totalDensity": total, "volume": header.unitVolume * n, "coordCenter": xyz(crs + s1 / np.maximum(n, 1)[:, None]),
            "centroid": xyz(crs + mean), "saddle": saddle, "prominence": np.abs(height.astype(np.float64)) - np.abs(saddle.astype(np.float64)),
            "neighbour": neighbour}


def groupBasins(columns, minProminence):
    """Shoulders joined to the peaks they lean on, in ONE pass -- not a persistence hierarchy: every peak with ``prominence <
    minProminence`` and a neighbour is joined to that neighbour (union-find over the edges i -> neighbour[i]); a group's representative
    is its smallest list index, i.e. its highest peak.  A low peak without a neighbour stays alone.  columns: ``basinFinish``'s.
    Returns ``{"representative" (per peak), "groups" (the representatives, ascending), "numVoxels", "totalDensity", "volume",
    "coordCenter", "centroid"}`` with one row per group for the last five: the sums of the members, the centres re-based from the
    members' absolute sums (n x coordCenter, |sum| x centroid)."""
    n = np.asarray(columns["numVoxels"], dtype=np.int64)
    count = len(n)
    neighbour, prominence = np.asarray(columns["neighbour"], dtype=np.int64), np.asarray(columns["prominence"], dtype=np.float64)
    parent = list(range(count))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i in np.nonzero((prominence < minProminence) & (neighbour >= 0))[0].tolist():
        a, b = find(i), find(int(neighbour[i]))
        if a != b:
            parent[max(a, b)] = min(a, b)          # (the smaller index stays the root: the representative is the group's minimum)
    representative = np.array([find(i) for i in range(count)], dtype=np.int64)
    groups, slot = np.unique(representative, return_inverse=True)
    total = np.asarray(columns["totalDensity"], dtype=np.float64)
    weight = np.abs(total)

    def fold(values):
        out = np.zeros((len(groups),) + np.shape(values)[1:], dtype=np.float64)
        np.add.at(out, slot, values)
        return out

    group_n, group_weight = fold(n.astype(np.float64)), fold(weight)
    with np.errstate(divide="ignore", invalid="ignore"):
        center = fold(np.asarray(columns["coordCenter"], dtype=np.float64) * n[:, None]) / group_n[:, None]
        centroid = np.where(group_weight[:, None] > 0, fold(np.asarray(columns["centroid"], dtype=np.float64) * weight[:, None]) / group_weight[:, None], center)
    return {"representative": representative, "groups": groups, "numVoxels": group_n.astype(np.int64), "totalDensity": fold(total),
            "volume": fold(np.asarray(columns["volume"], dtype=np.float64)), "coordCenter": center, "centroid": centroid}


SHAPE_COLUMNS = ("boxLo", "boxHi", "boxExtent", "onBorder", "extremeCrs", "extremeXyz", "extremeDensity", "weightedCentroid", "secondMomentCrs",
                 "weightedSecondMomentCrs", "secondMomentXyz", "weightedSecondMomentXyz", "principalLengths", "principalAxes", "weightedPrincipalLengths",
                 "weightedPrincipalAxes", "anisotropy", "equivalentRadii")
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # the order of the six second sums: cc cr cs rr rs ss


def _symmetric(six):
    """(n, 6) upper triangles in ``_PAIRS`` order -> (n, 3, 3) symmetric tensors."""
    out = np.zeros((len(six), 3, 3), dtype=np.float64)
    for k, (i, j) in enumerate(_PAIRS):
        out[:, i, j] = out[:, j, i] = six[:, k]
    return out


def _principal(tensor):
    """Batched ``eigh`` of (n, 3, 3) symmetric tensors: (lengths (n, 3) = sqrt of the principal variances, descending; axes (n, 3, 3), row k the
    unit vector of length k).  A tensor that holds a NaN (a blob without density has no weighted moments) gives NaN rows."""
    lengths, axes = np.full((len(tensor), 3), np.nan), np.full((len(tensor), 3, 3), np.nan)
    ok = np.isfinite(tensor).all(axis=(1, 2))
    if ok.any():
        values, vectors = np.linalg.eigh(tensor[ok])                  # ascending; vectors in columns
        lengths[ok] = np.sqrt(np.maximum(values[:, ::-1], 0.0))       # (a variance of a flat blob may come out as -1e-17)
        axes[ok] = np.transpose(vectors, (0, 2, 1))[:, ::-1, :]
    return lengths, axes


def blobShapeFinish(header, numVoxels, moments, wholeMap=False):
    """The shape columns of a blob list from the integer / fixed-point sums of ``pdbeda_bloblist_moments`` (``BlobList.moments()``) and the
    blobs' voxel counts -- a few vectorised fp64 operations per row, no voxel is touched.  A dict of arrays, one row per blob:

    ``boxLo`` / ``boxHi`` (raw crs, inclusive), ``boxExtent`` (the box's edges in A along the column, row and section axes: whole voxels,
    (hi - lo + 1) steps), ``onBorder`` (whole-map lists: the box touches a face of the non-repeating box ``header.uniqueNcrs`` -- the stored
    box begins at ``crsStart`` -- so the blob may go on in the next cell; False for every other list);
    ``extremeCrs`` / ``extremeXyz`` / ``extremeDensity`` (the voxel of largest |density| and its signed value);
    ``weightedCentroid`` (xyz of box_lo + sum w d / sum w, w = |density|);
    ``secondMomentCrs`` / ``weightedSecondMomentCrs`` ((n, 3, 3) central second moments of the voxel positions in voxels: the geometric one
    is (n sum d d' - sum d sum d') / n^2 with the numerator formed in exact integers) and the same in A^2, ``secondMomentXyz`` /
    ``weightedSecondMomentXyz`` = M C M^T with M the linear part of ``crs2xyzCoord`` (permuted axes and skewed cells included);
    ``principalLengths`` (RMS extent along the principal axes in A, descending) and ``principalAxes`` (row k: unit vector of length k) of
    the geometric tensor, ``weightedPrincipalLengths`` / ``weightedPrincipalAxes`` of the weighted one;
    ``anisotropy`` = 1 - l3 / l1 (0 for a single voxel) and ``equivalentRadii`` = sqrt(5) lengths: the semi-axes of the solid ellipsoid with
    these moments."""
    n = np.asarray(numVoxels, dtype=np.int64)
    count = len(n)
    s1, s2 = np.asarray(moments["s1"], dtype=np.int64).reshape(count, 3), np.asarray(moments["s2"], dtype=np.int64).reshape(count, 6)
    lo, hi = np.asarray(moments["boxLo"]).reshape(count, 3), np.asarray(moments["boxHi"]).reshape(count, 3)
    # n sum d d' - sum d sum d' in exact integers: int64 while every product stays below 2^62, Python integers beyond
    exact = np.int64 if count == 0 or (float(n.max()) * float(s2.max()) < 2.0 ** 62 and float(s1.max()) ** 2 < 2.0 ** 62) else object
    ne, s1e, s2e = n.astype(exact), s1.astype(exact), s2.astype(exact)
    numerator = np.stack([ne * s2e[:, k] - s1e[:, i] * s1e[:, j] for k, (i, j) in enumerate(_PAIRS)], axis=1) if count else np.zeros((0, 6))
    nn = (ne * ne).astype(np.float64) if count else np.zeros(0)
    geometric = _symmetric(numerator.astype(np.float64) / nn[:, None])
    sw = np.asarray(moments["sw"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.asarray(moments["sw1"], dtype=np.float64).reshape(count, 3) / sw[:, None]
        second = np.asarray(moments["sw2"], dtype=np.float64).reshape(count, 6) / sw[:, None]
    weighted = _symmetric(np.stack([second[:, k] - mean[:, i] * mean[:, j] for k, (i, j) in enumerate(_PAIRS)], axis=1) if count else np.zeros((0, 6)))
    M = (header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3)))).T          # column k: the xyz step of crs axis k
    geometricXyz, weightedXyz = np.einsum("ij,njk,lk->nil", M, geometric, M), np.einsum("ij,njk,lk->nil", M, weighted, M)
    lengths, axes = _principal(geometricXyz)
    weightedLengths, weightedAxes = _principal(weightedXyz)
    with np.errstate(divide="ignore", invalid="ignore"):
        anisotropy = np.where(lengths[:, 0] > 0, 1.0 - lengths[:, 2] / lengths[:, 0], 0.0)
    unique = np.asarray(header.uniqueNcrs, dtype=np.int64)
    border = ((lo <= 0) | (hi >= unique - 1)).any(axis=1) if wholeMap else np.zeros(count, dtype=bool)
    extremeCrs = np.asarray(moments["extremeCrs"]).reshape(count, 3)
    return {"boxLo": lo, "boxHi": hi, "boxExtent": (hi.astype(np.int64) - lo + 1) * np.linalg.norm(M, axis=0), "onBorder": border,
            "extremeCrs": extremeCrs, "extremeXyz": header.crs2xyz_array(extremeCrs).reshape(count, 3),
            "extremeDensity": np.asarray(moments["extreme"], dtype=np.float64), "weightedCentroid": header.crs2xyz_array(lo + mean).reshape(count, 3),
            "secondMomentCrs": geometric, "weightedSecondMomentCrs": weighted, "secondMomentXyz": geometricXyz, "weightedSecondMomentXyz": weightedXyz,
            "principalLengths": lengths, "principalAxes": axes, "weightedPrincipalLengths": weightedLengths, "weightedPrincipalAxes": weightedAxes,
            "anisotropy": anisotropy, "equivalentRadii": np.sqrt(5.0) * lengths}


NEAREST_MAX_OFFSETS, NEAREST_MAX_COMPONENT = 16384, 127      # what pdbeda_bloblist_nearest takes (its table lives in LDS as packed words)
NEAREST_COLUMNS = ("index", "partner", "distance", "voxel", "partnerVoxel", "voxelXyz", "partnerVoxelXyz")


def neighbourOffsets(header, maxDistance):
    """The ordered neighbourhood table of ``pdbeda_bloblist_nearest`` for a map: ``(offsets int32 (n, 3), distance float64 (n,))`` with every
    integer offset (dc, dr, ds) whose length |o . step| is <= ``maxDistance`` A -- step the linear part of ``crs2xyzCoord``, so permuted axes and
    skewed cells are included -- in ascending order of the squared length, ties by (dc, dr, ds) ascending, dc most significant.  The offset
    (0, 0, 0) comes first.  ValueError: more than 16384 offsets, or a component beyond +-127 (the limits of the device call).  Before it
    enumerates anything the function also refuses a reach whose bounding box of offsets holds more than 64 x 16384 candidates.  The
    ball fills pi / 6 of that box in an orthogonal cell and pi / 6 sin(angle) of it in a cell with one oblique angle, so a table that
    would fit is refused there only for cells skewed to within about 2 degrees of flat: none that a map comes with."""
    maxDistance = float(maxDistance)
    if not (maxDistance >= 0 and np.isfinite(maxDistance)):
        raise ValueError("maxDistance must be a finite, non-negative number of Angstrom")
    step = header.crs2xyz_array(np.eye(3)) - header.crs2xyz_array(np.zeros((1, 3)))          # row k: the xyz step of crs axis k
    # |o_k| <= |x| * |column k of step^-1| for x = o . step: the box that holds every offset of the ball
    reach = np.floor(maxDistance * np.linalg.norm(np.linalg.inv(step), axis=0) * (1.0 + 1e-12)).astype(np.int64) + 1
    if (reach - 1 > NEAREST_MAX_COMPONENT).any() or float(np.prod(2.0 * reach + 1.0)) > 64.0 * NEAREST_MAX_OFFSETS:
        raise ValueError("maxDistance = %g A reaches beyond the %d offsets of +-%d voxels that the nearest-blob search takes" %
                         (maxDistance, NEAREST_MAX_OFFSETS, NEAREST_MAX_COMPONENT))
    axes = [np.arange(-int(n), int(n) + 1, dtype=np.int64) for n in reach]
    cand = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    metric = step.dot(step.T)
    d2 = np.einsum("ni,ij,nj->n", cand.astype(np.float64), metric, cand.astype(np.float64))
    distance = np.sqrt(np.maximum(d2, 0.0))
    keep = distance <= maxDistance
    cand, d2, distance = cand[keep], d2[keep], distance[keep]
    if len(cand) > NEAREST_MAX_OFFSETS or (len(cand) and int(np.abs(cand).max()) > NEAREST_MAX_COMPONENT):
        raise ValueError("maxDistance = %g A gives %d offsets (the nearest-blob search takes %d of +-%d voxels)" %
                         (maxDistance, len(cand), NEAREST_MAX_OFFSETS, NEAREST_MAX_COMPONENT))
    order = np.lexsort((cand[:, 2], cand[:, 1], cand[:, 0], d2))
    return np.ascontiguousarray(cand[order], dtype=np.int32), np.ascontiguousarray(distance[order])


SPREAD_MAX_OFFSETS, SPREAD_MAX_REACH = _native.SPREAD_MAX_OFFSETS, _native.SPREAD_MAX_REACH      # PDBEDA_SPREAD_MAX_OFFSETS / _REACH of include/pdbeda.h

# Radii in Angstrom by element for the masks of ``DensityMatrix.atomMask`` / ``solventMask`` (van der Waals radii after Bondi, J. Phys. Chem. 68
# (1964) 441, hydrogen as the flat bulk-solvent model takes it); ``maskRadii`` gives any other element MASK_VDW_DEFAULT.
MASK_VDW = {"H": 1.2, "C": 1.7, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.8, "S": 1.8, "CL": 1.75, "SE": 1.9, "BR": 1.85, "I": 1.98,
            "NA": 2.27, "MG": 1.73, "K": 2.75, "CA": 2.31, "ZN": 1.39, "FE": 1.8, "MN": 1.8, "CU": 1.4, "NI": 1.63}
MASK_VDW_DEFAULT = 1.8


def maskRadii(elements):
    """MASK_VDW for a sequence of element symbols (any case, blanks ignored), MASK_VDW_DEFAULT for the others: float64 (n,)."""
    return np.array([MASK_VDW.get(str(e).strip().upper(), MASK_VDW_DEFAULT) for e in elements], dtype=np.float64)


def spreadTable(header, maxDistance):
    """``neighbourOffsets`` under the limits of ``pdbeda_map_spread``: ValueError for a component beyond +-32 or more than 16384 offsets.  In
    ascending distance a ball is searched row by row (every row of it falls to one minimum along dc and rises behind it)."""
    offsets, distance = neighbourOffsets(header, maxDistance)
    if len(offsets) > SPREAD_MAX_OFFSETS or (len(offsets) and int(np.abs(offsets).max()) > SPREAD_MAX_REACH):
        raise ValueError("maxDistance = %g A gives %d offsets of up to %d voxels (a spread takes %d of +-%d voxels)" %
                         (float(maxDistance), len(offsets), int(np.abs(offsets).max()), SPREAD_MAX_OFFSETS, SPREAD_MAX_REACH))
    return offsets, distance


def softEdgeValues(distance, radius, width):
    """The values of a soft-edged mask for a table's distances: float32 (n + 1,) -- 1 up to ``radius``, the raised cosine
    0.5 (1 + cos(pi (d - radius) / width)) down to 0 at ``radius + width``, and a last entry of 0 for no seed in reach."""
    d = np.asarray(distance, dtype=np.float64).reshape(-1)
    radius, width = float(radius), float(width)
    if not (radius >= 0 and width >= 0):
        raise ValueError("radius and width must be non-negative")
    out = np.where(d <= radius, 1.0, 0.0)
    if width > 0:
        edge = (d > radius) & (d < radius + width)
        out[edge] = 0.5 * (1.0 + np.cos(np.pi * (d[edge] - radius) / width))
    return np.append(out, 0.0).astype(np.float32)


class _DeviceBlobSegment(object):
    """One device blob list behind a ``DeviceBlobs`` sequence: its statistics columns and, once somebody asked, its objects."""

    def __init__(self, bl, densityMatrix, wholeMap=False):
        self.bl, self.densityMatrix, self.wholeMap = bl, densityMatrix, wholeMap
        self.stats = bl.stats()
        self.blobs = None
        self._shape = None

    def shape(self):
        """The shape columns of this list (``blobShapeFinish`` of ONE ``pdbeda_bloblist_moments`` call), made on first use."""
        if self._shape is None:
            self._shape = blobShapeFinish(self.densityMatrix.header, self.stats["n"], self.bl.moments(), self.wholeMap)
        return self._shape

    def __len__(self):
        return len(self.stats["n"])

    def made(self):
        if self.blobs is None:
            st, bl, densityMatrix = self.stats, self.bl, self.densityMatrix
            columns = zip(st["centroid"].tolist(), st["coordCenter"].tolist(), st["totalDensity"].tolist(), st["volume"].tolist(), st["n"].tolist(),
                          st["firstKey"].tolist())
            new = DensityBlob.__new__
            out = []
            for i, (centroid, center, total, volume, n, key) in enumerate(columns):
                blob = new(DensityBlob)                          # same fields as __init__ sets, without a call per field
                blob.__dict__ = {"centroid": centroid, "coordCenter": center, "totalDensity": total, "volume": volume, "_crsList": None, "_numVoxels": n,
                                 "_list": bl, "_index": i, "densityMatrix": densityMatrix, "firstKey": key, "_segment": self}
                out.append(blob)
            self.blobs = out
        return self.blobs


class DeviceBlobs(collections.abc.Sequence):
    """What ``createFullBlobList`` / ``findAberrantBlobs`` / ``createBlobList`` return (a list of DensityBlob in the reference,
    ccp4.py:463-485): the same blobs in the same order, as a read-only sequence whose objects are made on first access, one
    device list at a time.  ``a + b`` of two of them is again one (the objects are shared with ``a`` and ``b``); ``+`` with a
    plain list and ``==`` against one behave as a list's."""

    def __init__(self, segments):
        self._segments = list(segments)
        self._flat = None

    def __len__(self):
        return sum(len(seg) for seg in self._segments)

    def _all(self):
        if len(self._segments) == 1:
            return self._segments[0].made()
        if self._flat is None:       # (kept: the segments never change once the sequence exists, and an index loop must not rebuild it per access)
            self._flat = [blob for seg in self._segments for blob in seg.made()]
        return self._flat

    def __getitem__(self, i):
        return self._all()[i]

    def __iter__(self):
        return iter(self._all())

    def __add__(self, other):
        if isinstance(other, DeviceBlobs):
            return DeviceBlobs(self._segments + other._segments)
        return self._all() + other if isinstance(other, list) else NotImplemented

    def __radd__(self, other):
        return other + self._all() if isinstance(other, list) else NotImplemented

    def __eq__(self, other):
        if not isinstance(other, (list, DeviceBlobs)):
            return NotImplemented
        return len(self) == len(other) and all(a == b for a, b in zip(self, other))

    __hash__ = None

    def __repr__(self):
        return "DeviceBlobs(%d blobs)" % len(self)

    def voxelLists(self):
        """(crs[N, 3] int32 grouped by blob in list order, offsets[len + 1]): the voxels of every blob, a device list at a time."""
        parts = [seg.bl.voxels() for seg in self._segments]
        if not parts:
            return np.zeros((0, 3), dtype=np.int32), np.zeros(1, dtype=np.int64)
        offsets, base = [np.zeros(1, dtype=np.int64)], 0
        for crs, off in parts:
            offsets.append(off[1:] + base)
            base += len(crs)
        return np.concatenate([crs for crs, off in parts]), np.concatenate(offsets)

    def shapeColumns(self):
        """The shape of every blob, in list order: the ``SHAPE_COLUMNS`` of ``blobShapeFinish`` as arrays, from ONE device call per device
        list (``pdbeda_bloblist_moments`` in include/pdbeda.h has the contract) -- no voxel list comes to the host."""
        if not self._segments:
            return {k: np.zeros(0) for k in SHAPE_COLUMNS}
        parts = [seg.shape() for seg in self._segments]
        return parts[0] if len(parts) == 1 else {k: np.concatenate([part[k] for part in parts]) for k in SHAPE_COLUMNS}

    def nearestBlobs(self, other, maxDistance):
        """For every blob of this whole-map list the nearest blob of ``other`` -- the red list of the same ``createFullBlobLists`` call, a
        separately made list of the same map, or a list of another map on the same grid -- within ``maxDistance`` A, from ONE device call
        (``pdbeda_bloblist_nearest`` in include/pdbeda.h has the contract; the table is ``neighbourOffsets``): no label volume and no voxel
        list comes to the host.  A dict of arrays, one row per blob: ``partner`` (index in ``other``, -1 without one), ``distance`` (A between
        the two closest voxel centres, NaN without a partner), ``index`` (of that offset in the table), ``voxel`` / ``partnerVoxel`` (crs) and
        ``voxelXyz`` / ``partnerVoxelXyz``.  Among equally near pairs the table's order decides, then the c-major position of the voxel."""
        for blobs in (self, other):
            if not isinstance(blobs, DeviceBlobs) or len(blobs._segments) != 1 or not blobs._segments[0].wholeMap:
                raise ValueError("nearestBlobs works between two lists that createFullBlobList / createFullBlobLists returned (not joined ones)")
        mine, theirs = self._segments[0], other._segments[0]
        header = mine.densityMatrix.header
        offsets, distance = neighbourOffsets(header, maxDistance)
        out = mine.bl.nearest(theirs.bl, offsets)
        found = out["index"] >= 0
        out["distance"] = np.where(found, distance[np.where(found, out["index"], 0)], np.nan) if len(distance) else np.full(len(found), np.nan)
        out["voxelXyz"] = header.crs2xyz_array(out["voxel"]).reshape(-1, 3)
        out["partnerVoxelXyz"] = header.crs2xyz_array(out["partnerVoxel"]).reshape(-1, 3)
        return out

    def columns(self):
        """{"centroid", "totalDensity", "n", "volume"} of all blobs as arrays -- or None once any of the objects exists (they
        are ordinary mutable objects: from then on they are the truth)."""
        if any(seg.blobs is not None for seg in self._segments):
            return None
        if not self._segments:
            return {"centroid": np.zeros((0, 3)), "totalDensity": np.zeros(0), "n": np.zeros(0, dtype=np.int64), "volume": np.zeros(0)}
        return {k: np.concatenate([seg.stats[k] for seg in self._segments]) if len(self._segments) > 1 else self._segments[0].stats[k]
                for k in ("centroid", "totalDensity", "n", "volume")}


class DensityBlob(object):
    """A connected set of voxels with its fp64 statistics (ref ccp4.py:488-594).

    Blobs made by the device carry their statistics eagerly and their voxel set
    lazily (``crsList`` is fetched from the device label data on first use).
    """

    def __init__(self, centroid, coordCenter, totalDensity, volume, crsList, densityMatrix, atoms=None):
        self.centroid = centroid
        self.coordCenter = coordCenter
        self.totalDensity = totalDensity
        self.volume = volume
        self._crsList = None if crsList is None else {tuple(int(x) for x in crs) for crs in crsList}
        self._numVoxels = None
        self._list = None                  # blobs made by the device: the list handle and the position in it (voxels on demand)
        self._index = None
        self.densityMatrix = densityMatrix
        if atoms:
            self.atoms = atoms

    @classmethod
    def listFromDevice(cls, bl, densityMatrix, wholeMap=False):
        """The blobs of a device list, in its order: a sequence that makes the DensityBlob objects when somebody reads one
        (``DeviceBlobs``) -- the tables over thousands of blobs read the list's columns and never touch an object."""
        return DeviceBlobs([_DeviceBlobSegment(bl, densityMatrix, wholeMap)])

    def _shapeValue(self, name):
        segment = self.__dict__.get("_segment")
        if segment is None or self._list is None:
            raise AttributeError("%s is known only for a blob that comes from a device list (createFullBlobList, findAberrantBlobs, createBlobList) "
                                 "and has not been merged since" % name)
        value = segment.shape()[name][self._index]
        return value.tolist() if isinstance(value, np.ndarray) else value.item()

    @property
    def crsList(self):
        if self._crsList is None:
            self._crsList = {tuple(crs) for crs in self._list.voxels_of(self._index).tolist()}
        return self._crsList

    @property
    def atoms(self):
        """ref ccp4.py:505: the atoms a blob was built around (an empty list until somebody fills it)."""
        return self.__dict__.setdefault("_atoms", [])

    @atoms.setter
    def atoms(self, value):
        self.__dict__["_atoms"] = value

    @crsList.setter
    def crsList(self, value):
        self._crsList = value
        self._numVoxels = None

    @property
    def numVoxels(self):
        """``len(blob.crsList)`` without materialising the set."""
        if self._crsList is not None:
            return len(self._crsList)
        return self._numVoxels

    @property
    def validCrs(self):
        """ref ccp4.py:518-520 -> cutils.pyx:169-183."""
        crs = np.asarray(sorted(self.crsList), dtype=np.int32).reshape(-1, 3)
        return bool(self.densityMatrix._map.valid_crs(crs).all())

    @staticmethod
    def fromCrsList(crsList, densityMatrix):
        """ref ccp4.py:522-545: statistics of an explicit voxel set (computed on the device)."""
        crs = np.asarray([list(c) for c in crsList], dtype=np.int32).reshape(-1, 3)
        st = densityMatrix._map.list_stats(crs)
        return DensityBlob(list(st["centroid"]), list(st["coordCenter"]), float(st["totalDensity"]), float(st["volume"]),
                           crs, densityMatrix)

    def __eq__(self, otherBlob):
        """ref ccp4.py:548-562."""
        if abs(self.volume - otherBlob.volume) >= 1e-6:
            return False
        if abs(self.totalDensity - otherBlob.totalDensity) >= 1e-6:
            return False
        return all(abs(self.centroid[i] - otherBlob.centroid[i]) < 1e-6 for i in range(3))

    __hash__ = None

    def testOverlap(self, otherBlob):
        """ref ccp4.py:564-573 -> cutils.pyx:8-25: any voxel pair at Chebyshev distance <= 1."""
        a = np.asarray(sorted(self.crsList), dtype=np.int32).reshape(-1, 3)
        b = np.asarray(sorted(otherBlob.crsList), dtype=np.int32).reshape(-1, 3)
        return bool(self.densityMatrix._map.test_overlap(a, b))

    def merge(self, otherBlob):
        """ref ccp4.py:575-586: set union, statistics recomputed over the union."""
        union = set(self.crsList) | set(otherBlob.crsList)
        atoms = self.atoms + [atom for atom in otherBlob.atoms if atom not in self.atoms]
        new = DensityBlob.fromCrsList(sorted(union), self.densityMatrix)
        self.centroid, self.coordCenter = new.centroid, new.coordCenter
        self.totalDensity, self.volume = new.totalDensity, new.volume
        self._crsList, self._numVoxels, self._list, self._index = new._crsList, None, None, None
        self.atoms = atoms

    def clone(self):
        """ref ccp4.py:588-594."""
        return DensityBlob(self.centroid, self.coordCenter, self.totalDensity, self.volume, self.crsList,
                           self.densityMatrix, self.atoms.copy())


def _shapeAttribute(name):
    return property(lambda self: self._shapeValue(name), doc="``%s`` of ``blobShapeFinish`` for this blob (read-only; made on first use for the whole list)." % name)


for _name in SHAPE_COLUMNS:
    setattr(DensityBlob, _name, _shapeAttribute(_name))


def _basinAttribute(name):
    return property(lambda self: self._basinValue(name), doc="``%s`` of ``basinFinish`` for this peak (read-only; made on first use for the whole list)." % name)


for _name in BASIN_COLUMNS:
    setattr(DensityPeak, _name, _basinAttribute(_name))
del _name
