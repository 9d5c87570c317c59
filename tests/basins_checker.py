"""Plain numpy restatement of the peak-basin contract (include/pdbeda.h, pdbeda_peaklist_basins) -- the yardstick of the basin
tests.  It shares no code with the library: every voxel gets its rank under the total order of the peak search, the parent of a
significant voxel is the 27-shift minimum of the ranks of the significant voxels around it, roots come by pointer doubling, sums
by ``bincount`` and saddles by ``np.maximum.at`` over the 13 offset pairs.  The order of the rows is ``peaks_checker.find_peaks``'."""
import itertools

import numpy as np

import peaks_checker


def find_basins(header, grid, cutoff):
    """grid: float32 [ns][nr][nc] as stored.  Returns a dict: per peak (list order) ``n``, ``sum``, ``s1`` (n x 3), ``sw1`` (n x 3),
    ``saddle`` (float32), ``neighbour`` (int32), ``maxd`` (largest |d| of the basin); ``basin`` int32 [us][ur][uc]; ``significant``,
    ``orphans``, ``steps`` (longest ascent, in parent steps) and ``peaks`` (the checker's peak rows)."""
    t = np.float32(cutoff)
    peaks = peaks_checker.find_peaks(header, grid, cutoff)
    uc, ur, us = (int(v) for v in header.uniqueNcrs)
    box = np.ascontiguousarray(np.asarray(grid, dtype=np.float32)[:us, :ur, :uc])
    D = np.ascontiguousarray(np.transpose(box, (2, 1, 0)))                              # D[c, r, s]: flat index = c-major position
    nvox = D.size
    with np.errstate(invalid="ignore"):
        sig = (D >= t) if t > 0 else (D <= t)                                          # inclusive; NaN fails
    mag = np.where(sig, np.abs(D), np.float32(0)).astype(np.float32).ravel()
    # rank 0 = the voxel that beats every other: descending |D|, ties by c-major position (the flat index)
    order = np.lexsort((np.arange(nvox), -mag.astype(np.float64)))
    rank = np.empty(nvox, dtype=np.int64)
    rank[order] = np.arange(nvox)
    NONE = np.int64(nvox)
    rank = np.where(sig.ravel(), rank, NONE).reshape(D.shape)
    pad = np.full((uc + 2, ur + 2, us + 2), NONE, dtype=np.int64)
    pad[1:-1, 1:-1, 1:-1] = rank
    best = rank.copy()
    for dc, dr, ds in itertools.product((-1, 0, 1), repeat=3):
        best = np.minimum(best, pad[1 + dc:1 + dc + uc, 1 + dr:1 + dr + ur, 1 + ds:1 + ds + us])
    flat_sig = np.nonzero(sig.ravel())[0]
    up = np.arange(nvox, dtype=np.int64)
    up[flat_sig] = order[best.ravel()[flat_sig]]                                       # rank -> voxel
    # pointer doubling; depth[v] counts the parent steps from v to up[v] on the way
    depth = (up != np.arange(nvox)).astype(np.int64)
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        depth = depth + depth[up]
        up = nxt
    longest = int(depth.max()) if nvox else 0
    n_peaks = len(peaks["crs"])
    index_of = np.full(nvox, -1, dtype=np.int64)
    index_of[peaks["key"]] = np.arange(n_peaks)
    basin = np.full(nvox, -1, dtype=np.int64)
    basin[flat_sig] = index_of[up[flat_sig]]
    member = np.nonzero(basin >= 0)[0]
    b = basin[member]
    c, r, s = np.unravel_index(member, D.shape)
    crs = np.stack([c, r, s], axis=1).astype(np.int64)
    d = crs - peaks["crs"].astype(np.int64)[b]
    rho = D.ravel()[member].astype(np.float64)
    fin = np.isfinite(rho)
    n = np.bincount(b, minlength=n_peaks).astype(np.int64)
    total = np.bincount(b[fin], weights=rho[fin], minlength=n_peaks)
    s1 = np.stack([np.bincount(b, weights=d[:, k], minlength=n_peaks) for k in range(3)], axis=1).astype(np.int64)
    sw1 = np.stack([np.bincount(b[fin], weights=np.abs(rho[fin]) * d[fin, k], minlength=n_peaks) for k in range(3)], axis=1)
    maxd = np.zeros(n_peaks, dtype=np.int64)
    if len(member):
        np.maximum.at(maxd, b, np.abs(d).max(axis=1))
    # saddles: every unordered pair of neighbours once (13 offsets), both directions of it
    B = basin.reshape(D.shape)
    bits = np.abs(D).view(np.uint32).astype(np.uint64)
    key = np.zeros(n_peaks, dtype=np.uint64)
    for off in itertools.product((-1, 0, 1), repeat=3):
        if off <= (0, 0, 0):
            continue
        lo = tuple(slice(max(0, -o), dim - max(0, o)) for o, dim in zip(off, D.shape))
        hi = tuple(slice(max(0, o), dim - max(0, -o)) for o, dim in zip(off, D.shape))
        bp, bq = B[lo], B[hi]
        pair = (bp >= 0) & (bq >= 0) & (bp != bq)
        if not pair.any():
            continue
        pass_bits = np.minimum(bits[lo][pair], bits[hi][pair])
        p_i, q_i = bp[pair].astype(np.uint64), bq[pair].astype(np.uint64)
        np.maximum.at(key, bp[pair], (pass_bits << np.uint64(32)) | (np.uint64(0xffffffff) - q_i))
        np.maximum.at(key, bq[pair], (pass_bits << np.uint64(32)) | (np.uint64(0xffffffff) - p_i))
    has = key != 0
    neighbour = np.where(has, (np.uint64(0xffffffff) - (key & np.uint64(0xffffffff))).astype(np.int64), -1).astype(np.int32)
    saddle_bits = (key >> np.uint64(32)).astype(np.uint32)
    if t < 0:
        saddle_bits = np.where(has, saddle_bits | np.uint32(0x80000000), saddle_bits).astype(np.uint32)
    saddle = saddle_bits.view(np.float32)
    volume = np.ascontiguousarray(np.transpose(B, (2, 1, 0))).astype(np.int32)          # [s][r][c]
    return {"n": n, "sum": total, "s1": s1, "sw1": sw1, "saddle": saddle, "neighbour": neighbour, "maxd": maxd, "basin": volume,
            "significant": int(len(flat_sig)), "orphans": int(len(flat_sig) - len(member)), "steps": longest, "peaks": peaks}
