"""The numpy restatement of crystal contacts the GPU tests check against (pdb_eda_amd/crystalContacts.py states the definition),
and the synthetic crystals they run on.  Distances are scipy cdist's: sqrt((dx*dx + dy*dy) + dz*dz) in fp64; an image coordinate is
((r0*x + r1*y) + r2*z + t) + orthoMat.n with orthoMat.n as the device's matvec3 computes it (two fma).  Large sets find their
candidate pairs with ``scipy.spatial.cKDTree`` at cutoff + 0.01 and recompute the exact formula on those pairs only."""
import numpy as np

from pdb_eda_amd import ccp4

KD_SLACK = 0.01


def ortho_times(ortho, n):
    """matvec3 (pdbeda_device.h): out[i] = fma(a[i][2], v[2], fma(a[i][0], v[0], a[i][1] * v[1]))."""
    a = np.asarray(ortho, dtype=np.float64).reshape(3, 3)
    v = [float(x) for x in n]
    return np.array([ccp4._fma(a[i, 2], v[2], ccp4._fma(a[i, 0], v[0], a[i, 1] * v[1])) for i in range(3)])


def image(rot, ortho, cand, p):
    """g(p) for the image cand = (op, n0, n1, n2): ((r0 x + r1 y) + r2 z + t) + orthoMat n, column by column."""
    m = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 4)[int(cand[0])]
    ot = ortho_times(ortho, cand[1:4])
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(p)
    for q in range(3):
        w = (m[q, 0] * p[:, 0] + m[q, 1] * p[:, 1]) + m[q, 2] * p[:, 2]
        out[:, q] = (w + m[q, 3]) + ot[q]
    return out


def pair_dist(a, b):
    d = a - b
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def min_dist_brute(q, p):
    """min over p of |q - p| for every q (fp64, cdist's formula), in blocks."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    out = np.full(len(q), np.inf)
    if len(p) == 0:
        return out
    for s in range(0, len(q), 256):
        out[s:s + 256] = pair_dist(q[s:s + 256, None, :], p[None, :, :]).min(axis=1)
    return out


def min_dist_kd(q, p, cutoff):
    """min over p of |q - p| where it is <= cutoff (inf elsewhere): candidate pairs by cKDTree, then the exact formula."""
    from scipy.spatial import cKDTree
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    out = np.full(len(q), np.inf)
    if len(p) == 0 or len(q) == 0:
        return out
    lists = cKDTree(p).query_ball_point(q, cutoff + KD_SLACK, return_sorted=False)
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(q))
    if lens.sum() == 0:
        return out
    qi = np.repeat(np.arange(len(q)), lens)
    pj = np.fromiter((j for x in lists for j in x), dtype=np.int64, count=int(lens.sum()))
    d = pair_dist(q[qi], p[pj])
    np.minimum.at(out, qi, d)
    return out


def coord_contacts(q, p, cutoff, kd=False):
    """findCoordContacts: (index, distance) arrays of the queries whose minimum distance is <= cutoff."""
    d = min_dist_kd(q, p, cutoff) if kd else min_dist_brute(q, p)
    idx = np.nonzero(d <= cutoff)[0]
    return idx.astype(np.int64), d[idx]


def kept_images(rot, ortho, poly, cand, cutoff):
    """Keep flag of every candidate image: some g(x_j) within cutoff of some x_i."""
    from scipy.spatial import cKDTree
    poly = np.asarray(poly, dtype=np.float64).reshape(-1, 3)
    tree = cKDTree(poly)
    lo, hi = poly.min(axis=0) - cutoff - 1.0, poly.max(axis=0) + cutoff + 1.0
    keep = np.zeros(len(cand), dtype=bool)
    for c, k in enumerate(np.asarray(cand)):
        img = image(rot, ortho, k, poly)
        near = img[np.all((img >= lo) & (img <= hi), axis=1)]
        if len(near) == 0:
            continue
        lists = tree.query_ball_point(near, cutoff + KD_SLACK, return_sorted=False)
        for a, js in enumerate(lists):
            if js and pair_dist(near[a][None, :], poly[js]).min() <= cutoff:
                keep[c] = True
                break
    return keep


def kept_images_diag(ortho_diag, poly, cand, cutoff):
    """kept_images for the identity operator and a diagonal cell with whole-number edges, vectorised over the candidates (every atom pair
    is tried: few atoms, any number of candidates).  orthoMat.n is then the exact product n * a (no fma is needed to state it), and the
    image coordinate ((1 x + 0 y) + 0 z + 0) + n a is x + n a."""
    a = np.asarray(ortho_diag, dtype=np.float64).reshape(3)
    poly = np.asarray(poly, dtype=np.float64).reshape(-1, 3)
    cand = np.asarray(cand).reshape(-1, 4)
    assert np.all(cand[:, 0] == 0) and np.all(a == np.round(a)) and float(np.abs(cand[:, 1:]).max(initial=0)) * a.max() < 2.0 ** 53
    ot = cand[:, 1:4].astype(np.float64) * a
    keep = np.zeros(len(cand), dtype=bool)
    for xj in poly:
        img = ((xj + 0.0) + 0.0) + ot
        for xi in poly:
            keep |= pair_dist(img, xi) <= cutoff
    return keep


def neighbours(rot, ortho, poly, images):
    """N in (image, atom) order."""
    if len(images) == 0:
        return np.zeros((0, 3))
    return np.concatenate([image(rot, ortho, k, poly) for k in np.asarray(images)])


def crystal_contacts(query, rot, ortho, poly, cand, cutoff, kd=True):
    """(keep flags, index, distance) of the whole definition."""
    keep = kept_images(rot, ortho, poly, cand, cutoff)
    n = neighbours(rot, ortho, poly, np.asarray(cand)[keep])
    idx, dist = coord_contacts(query, n, cutoff, kd=kd)
    return keep, idx, dist


# ---- synthetic crystals -----------------------------------------------------------------------------------------------------------------
def ortho_matrix(cell, angles):
    """The cell's orthoMat as the CCP4 header computes it (ccp4.DensityHeader)."""
    from pdb_eda_amd import synthetic
    spec = synthetic.MapSpec(ncrs=(16, 16, 16), cell=cell, angles=angles)
    return np.asarray(ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(spec)).orthoMat, dtype=np.float64)


def _frac_ops(group):
    """(rotation in fractional coordinates, fractional translation) of the space group's general positions."""
    I = np.eye(3)
    if group == "P1":
        return [(I, (0, 0, 0))]
    if group == "P212121":
        return [(I, (0, 0, 0)), (np.diag([-1, -1, 1]), (0.5, 0, 0.5)), (np.diag([-1, 1, -1]), (0, 0.5, 0.5)), (np.diag([1, -1, -1]), (0.5, 0.5, 0))]
    if group == "C2":
        two = np.diag([-1, 1, -1])
        return [(I, (0, 0, 0)), (two, (0, 0, 0)), (I, (0.5, 0.5, 0)), (two, (0.5, 0.5, 0))]
    if group == "P61":
        r6 = np.array([[1, -1, 0], [1, 0, 0], [0, 0, 1]])
        ops, r = [], np.eye(3)
        for k in range(6):
            ops.append((r.copy(), (0, 0, k / 6.0)))
            r = r6.dot(r)
        return ops
    raise ValueError(group)


CELLS = {"P1": ((38.0, 41.0, 45.0), (80.0, 95.0, 105.0)), "P212121": ((40.0, 46.0, 52.0), (90.0, 90.0, 90.0)),
         "C2": ((70.0, 36.0, 44.0), (90.0, 108.0, 90.0)), "P61": ((36.0, 36.0, 90.0), (90.0, 90.0, 120.0))}


def smtry(group, ortho):
    """The REMARK 290 SMTRY operators (Cartesian, 3 x 4) as a PDB file prints them: rotations to 6 decimals, translations to 5."""
    o = np.asarray(ortho, dtype=np.float64)
    oi = np.linalg.inv(o)
    out = []
    for r, t in _frac_ops(group):
        rc = np.round(o.dot(np.asarray(r, dtype=np.float64)).dot(oi), 6)
        tc = np.round(o.dot(np.asarray(t, dtype=np.float64)), 5)
        out.append(np.hstack([rc + 0.0, (tc + 0.0)[:, None]]))
    return out


def blob(n_atoms, seed, lo, hi):
    """n_atoms random points in the box [lo, hi] at PDB precision (3 decimals)."""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(lo, hi, (n_atoms, 3)), 3)


def crystal(group, n_atoms=400, seed=0, outside=3.0):
    """(rot (list of 3 x 4), ortho, polymer coordinates) of a small crystal: random atoms in a box a little smaller than the cell that
    reaches ``outside`` A beyond the cell's origin corner."""
    cell, angles = CELLS[group]
    ortho = ortho_matrix(cell, angles)
    return smtry(group, ortho), ortho, blob(n_atoms, seed, -outside, 0.97 * min(cell) - outside)
