"""A plain numpy restatement of the contract of pdbeda_bloblist_nearest (include/pdbeda.h).  For t in table order the mask of list b is
shifted by the offset INSIDE the box (nothing wraps) and the first t is recorded per voxel of list a; then per blob of a the minimum of
(t, c-major position).  Everything is an integer: the product's columns are compared with ``np.array_equal``."""
import numpy as np


def labels_of(shape, crs, offsets):
    """The label volume [s][r][c] (blob index or -1) of voxel lists: crs (N, 3) grouped by blob, offsets (blobs + 1)."""
    lab = np.full(shape, -1, dtype=np.int64)
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    counts = np.diff(np.asarray(offsets, dtype=np.int64))
    lab[crs[:, 2], crs[:, 1], crs[:, 0]] = np.repeat(np.arange(len(counts)), counts)
    return lab


def first_hit(labels_a, labels_b, table):
    """Per voxel [s][r][c]: the first t with a voxel of b at voxel + table[t] inside the box, or -1 (only where a has a voxel)."""
    ns, nr, nc = labels_a.shape
    in_a, in_b = labels_a >= 0, labels_b >= 0
    first = np.full(labels_a.shape, -1, dtype=np.int64)
    open_ = in_a.copy()
    for t, (dc, dr, ds) in enumerate(np.asarray(table, dtype=np.int64).reshape(-1, 3).tolist()):
        if not open_.any():
            break
        if abs(dc) >= nc or abs(dr) >= nr or abs(ds) >= ns:
            continue
        # hit[s, r, c] = in_b[s + ds, r + dr, c + dc] where that lies inside the box
        hit = np.zeros_like(in_b)
        dst = tuple(slice(max(0, -d), n - max(0, d)) for d, n in ((ds, ns), (dr, nr), (dc, nc)))
        src = tuple(slice(max(0, d), n - max(0, -d)) for d, n in ((ds, ns), (dr, nr), (dc, nc)))
        hit[dst] = in_b[src]
        new = open_ & hit
        first[new] = t
        open_ &= ~new
    return first


def nearest(labels_a, labels_b, table, count_a):
    """The four columns of the contract for the ``count_a`` blobs of a."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 3)
    ns, nr, nc = labels_a.shape
    first = first_hit(labels_a, labels_b, table)
    out = {"index": np.full(count_a, -1, np.int32), "partner": np.full(count_a, -1, np.int32), "voxel": np.zeros((count_a, 3), np.int32),
           "partnerVoxel": np.zeros((count_a, 3), np.int32)}
    s, r, c = np.nonzero(first >= 0)
    if len(s) == 0:
        return out
    blob, t = labels_a[s, r, c], first[s, r, c]
    position = (c.astype(np.int64) * nr + r) * ns + s                       # c-major: c most significant (first_key of pdbeda_bloblist_stats)
    order = np.lexsort((position, t, blob))
    lead = order[np.concatenate([[True], np.diff(blob[order]) != 0])]          # the smallest (t, position) of every blob that has a pair
    for k in lead.tolist():
        i, p = int(blob[k]), np.array([c[k], r[k], s[k]], dtype=np.int64)
        q = p + table[t[k]]
        out["index"][i], out["voxel"][i], out["partnerVoxel"][i] = t[k], p, q
        out["partner"][i] = labels_b[q[2], q[1], q[0]]
    return out
