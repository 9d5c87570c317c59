"""DensityAnalysis.aggregateCloud up to its statistics tail (densityAnalysis.py:571-731) restated on the flattened arrays of
``pdbeda_cloud_atoms``, with sets of voxel tuples and dicts: the yardstick of the small cases of tests/test_cloud_host.py and
tests/test_gpu_cloud.py.  Nothing is shared with the native library or with oracle/pdbeda_oracle.c except the per-atom clouds
themselves (``Oracle.find_aberrant_blobs``, pinned on the reference's goldens), the wrapped fetch of tests/profiles_checker.py
and the header's crs2xyz_array.

``mutate`` reruns the restatement with ONE rule changed, so that a case can show that it tells the rule from its neighbour:
"six" (6-connectivity for 26, in testOverlap and in the unions), "gt" (> for >= min_cloud_electrons), "last_min" (the last
minimum among the centroid distances for the first), "first_key" (the first pooled atom of a key for the last), "both_alias"
(two atoms of one residue that share a coordinate both named by their clouds), "no_cut" (no atom dropped by the centroid-distance
cut-off)."""
import itertools

import numpy as np

import profiles_checker

NEAR26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
NEAR6 = [d for d in NEAR26 if sum(abs(x) for x in d) == 1]


def atom_clouds(oracle, xyz, radius, cutoff):
    """Per atom: [(frozenset of raw crs tuples, totalDensity, centroid)] in the list order of findAberrantBlobs."""
    out = []
    for p, r in zip(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(radius, dtype=np.float32)):
        out.append([(frozenset(tuple(int(x) for x in v) for v in b["crs"]), float(b["totalDensity"]), np.array(b["centroid"], dtype=np.float64))
                    for b in oracle.find_aberrant_blobs([p], [r], cutoff)])
    return out


def voxel_stats(header, grid, voxels):
    """totalDensity and centroid of a set of raw crs tuples (DensityBlob.fromCrsList), summed in sorted order."""
    crs = np.array(sorted(voxels), dtype=np.int64).reshape(-1, 3)
    rho, _ = profiles_checker.point_density(header, grid, crs)
    where = header.crs2xyz_array(crs)          # (crs2xyzCoord on an array)
    total = float(np.sum(rho))
    return total, (rho[:, None] * where).sum(axis=0) / total


def touches(a, b, near):
    """utils.testOverlap: some voxel of a and some voxel of b within 1 on every axis (equal voxels included)."""
    small, large = (a, b) if len(a) <= len(b) else (b, a)
    return any(v in large or any((v[0] + d[0], v[1] + d[1], v[2] + d[2]) in large for d in near) for v in small)


def components(voxels, near):
    """The connected components of a voxel set, breadth first: a list of sets."""
    left, out = set(voxels), []
    while left:
        seed = left.pop()
        comp, frontier = {seed}, [seed]
        while frontier:
            nxt = []
            for v in frontier:
                for d in near:
                    w = (v[0] + d[0], v[1] + d[1], v[2] + d[2])
                    if w in left:
                        left.discard(w); comp.add(w); nxt.append(w)
            frontier = nxt
        out.append(comp)
    return out


def _rows(header, grid, pool, near, min_electrons, strict, weight, residue_of_entry):
    """pool: [(voxel set, named atom)] in pool order.  The union components, each with the distinct atoms its pooled clouds name,
    ordered by their lowest pool entry: (rows that pass the filter, all rows)."""
    comps = components(set().union(*[v for v, _ in pool]) if pool else set(), near)
    comp_of = {v: k for k, comp in enumerate(comps) for v in comp}
    entries = [[] for _ in comps]
    for q, (v, _) in enumerate(pool):
        entries[comp_of[min(v)]].append(q)
    found = []
    for comp, inside in zip(comps, entries):
        atoms = sorted({pool[q][1] for q in inside})
        total, centroid = voxel_stats(header, grid, comp)
        found.append({"first": inside[0], "residue": residue_of_entry[inside[0]], "n": len(comp), "total": total, "centroid": centroid,
                      "electrons": float(sum(weight[a] for a in atoms))})
    found.sort(key=lambda r: r["first"])
    keep = [r for r in found if (r["electrons"] > min_electrons if strict else r["electrons"] >= min_electrons)]
    return keep, found


def aggregate_cloud(header, grid, clouds, xyz, weight, residue, alias, key, bonded_off, bonded, owner_key, min_cloud_electrons, mutate=None):
    """The result dict of DeviceMap.aggregate_cloud; ``clouds`` = atom_clouds() of the same atoms."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n, near = len(xyz), NEAR6 if mutate == "six" else NEAR26
    dist = [[float(np.linalg.norm(xyz[i] - c[2])) for c in clouds[alias[i]]] for i in range(n)]
    own = [min(float(np.linalg.norm(xyz[i] - c[2])) for c in clouds[i]) for i in range(n) if clouds[i]]
    cut = float(np.median(own) + 2.5 * np.std(own)) if own else float("nan")
    atom_rows, res_rows, everything, everything_res = [], [], [], []
    owner_state = np.zeros(len(owner_key), dtype=np.uint8)
    for r in sorted(set(int(x) for x in residue)):
        pool, entries_of_key, named = [], {}, {}
        for i in [i for i in range(n) if residue[i] == r]:
            mine = clouds[alias[i]]
            if not mine or (len(mine) > 1 and min(dist[i]) > cut and mutate != "no_cut"):
                continue
            best = dist[i].index(min(dist[i])) if mutate != "last_min" else len(dist[i]) - 1 - dist[i][::-1].index(min(dist[i]))
            if not (mutate == "first_key" and key[i] in entries_of_key):
                entries_of_key[int(key[i])] = range(len(pool), len(pool) + len(mine))
            for c in range(len(mine)):
                pool.append(((int(alias[i]), c), i))
                if mutate != "both_alias":
                    named[(int(alias[i]), c)] = i          # the clouds of a coordinate are shared objects: they name the LAST atom pooled
            atom_rows.append((i, mine[best][1], len(mine[best][0]), mine[best][2], dist[i][best]))
        pool = [(clouds[obj[0]][obj[1]][0], named.get(obj, i)) for obj, i in pool]
        for o, k in enumerate(owner_key):
            if int(k) in entries_of_key:
                partners = [int(k2) for k2 in bonded[bonded_off[k]:bonded_off[k + 1]] if int(k2) in entries_of_key]
                ok = all(any(p != q and touches(pool[p][0], pool[q][0], near) for p in entries_of_key[int(k)] for q in entries_of_key[k2]) for k2 in partners)
                owner_state[o] = 1 if ok else 2
        keep, _ = _rows(header, grid, pool, near, min_cloud_electrons, mutate == "gt", weight, [r] * len(pool))
        res_rows += keep
        everything += pool
        everything_res += [r] * len(pool)
    dom_rows, dom_all = _rows(header, grid, everything, near, min_cloud_electrons, mutate == "gt", weight, everything_res)

    def table(rows):
        return {"residue": np.array([x["residue"] for x in rows], dtype=np.int32), "total": np.array([x["total"] for x in rows], dtype=np.float64),
                "n": np.array([x["n"] for x in rows], dtype=np.int64), "electrons": np.array([x["electrons"] for x in rows], dtype=np.float64),
                "centroid": np.array([x["centroid"] for x in rows], dtype=np.float64).reshape(-1, 3)}
    return {"numVoxels": int(sum(x["n"] for x in dom_all)), "totalElectrons": float(sum(x["electrons"] for x in dom_all)),
            "totalDensity": float(sum(x["total"] for x in dom_all)), "centroidDistanceCutoff": cut, "owner_state": owner_state,
            "atom": np.array([a[0] for a in atom_rows], dtype=np.int32), "atom_total": np.array([a[1] for a in atom_rows], dtype=np.float64),
            "atom_n": np.array([a[2] for a in atom_rows], dtype=np.int64), "atom_centroid": np.array([a[3] for a in atom_rows], dtype=np.float64).reshape(-1, 3),
            "atom_distance": np.array([a[4] for a in atom_rows], dtype=np.float64), "res": table(res_rows), "dom": table(dom_rows)}


def union_job(header, grid, clouds, pool_cloud, pool_group, n_groups, pair_a, pair_b, near=NEAR26):
    """What the device delivers to the host between the two halves of pdbeda_aggregate_cloud's decisions (pdb_eda_amd/csrc/pdbeda_cloud.h), made
    with the functions above.  ``clouds`` = atom_clouds(); a pooled cloud is a row of the clouds' table, which lists them atom by atom in list
    order.  The union job has a group per residue group of the pool (``pool_group``) and the domain group n_groups - 1, which holds every pooled
    voxel.  Returns u_n, u_total, u_centroid, u_group -- a row per connected component of a group's voxels, in no particular order --, comp
    (2 x pool entries: the row that holds the entry's voxels in its residue group, then in the domain group) and touch (a flag per pair: the
    voxels of all clouds of atom pair_a and those of atom pair_b touch)."""
    flat = [c[0] for mine in clouds for c in mine]
    rows, comp = [], np.full((2, len(pool_cloud)), -1, dtype=np.int32)
    for g in range(n_groups):
        kind = int(g == n_groups - 1)
        inside = [p for p in range(len(pool_cloud)) if kind or pool_group[p] == g]
        found = components(set().union(*[flat[pool_cloud[p]] for p in inside]) if inside else set(), near)
        row_of = {v: len(rows) + k for k, part in enumerate(found) for v in part}
        for p in inside:
            comp[kind, p] = row_of[min(flat[pool_cloud[p]])]
        rows += [(len(part),) + voxel_stats(header, grid, part) + (g,) for part in found]
    everything = [set().union(*[c[0] for c in mine]) if mine else set() for mine in clouds]
    touch = np.array([touches(everything[a], everything[b], near) for a, b in zip(pair_a, pair_b)], dtype=np.uint32)
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows], dtype=np.float64).reshape(-1, 3), np.array([r[3] for r in rows], dtype=np.int32), comp.reshape(-1), touch)


def assert_same_tables(got, want, exact=False, ordered=True, what=""):
    """Every row of every table of two aggregate_cloud results.  Counts, atom indices, voxel counts, owner states, residue ordinals
    and numVoxels are exact; electrons and the cut-off agree to 1e-12, densities and centroids to 1e-9 relative (1e-9 absolute on
    centroids), distances to 1e-8 / 1e-10 -- the project's tolerances for this comparison (the fixed-point quantum of the blob sums is
    at most 2^-36 of max |rho| a voxel).  exact: dyadic densities on voxel centres -- densities and electrons with ==, centroids and
    distances at 1e-12.  ordered: the residue rows in the order the ABI fixes; else sorted by (residue, voxels, density) like the domain
    rows, whose order the ABI leaves open."""
    rel, cen_abs, dist = (0.0, 1e-12, (1e-12, 1e-12)) if exact else (1e-9, 1e-9, (1e-8, 1e-10))
    close = lambda a, b, r, t=0.0: a.shape == b.shape and bool(np.all(np.abs(a - b) <= t + r * np.abs(b)))
    assert got["numVoxels"] == want["numVoxels"], what
    assert close(np.float64(got["totalElectrons"]), np.float64(want["totalElectrons"]), 0.0 if exact else 1e-12), what
    assert close(np.float64(got["totalDensity"]), np.float64(want["totalDensity"]), rel), what
    a, b = got["centroidDistanceCutoff"], want["centroidDistanceCutoff"]
    assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * abs(b), (what, a, b)
    for f in ("atom", "atom_n", "owner_state"):
        assert np.array_equal(got[f], want[f]), (what, f)
    assert close(got["atom_total"], want["atom_total"], rel), what
    assert close(got["atom_centroid"], want["atom_centroid"], 0.0 if exact else 1e-9, cen_abs), what
    assert close(got["atom_distance"], want["atom_distance"], dist[0], dist[1]), what
    for tag in ("res", "dom"):
        g, w = got[tag], want[tag]
        assert len(g["n"]) == len(w["n"]), (what, tag, len(g["n"]), len(w["n"]))
        if tag == "res" and ordered:
            kg = kw = np.arange(len(g["n"]))
        else:
            kg, kw = row_order(g, tag), row_order(w, tag)
        assert np.array_equal(g["n"][kg], w["n"][kw]), (what, tag)
        if tag == "res":
            assert np.array_equal(g["residue"][kg], w["residue"][kw]), (what, tag)
        assert close(g["total"][kg], w["total"][kw], rel), (what, tag)
        assert close(g["electrons"][kg], w["electrons"][kw], 0.0 if exact else 1e-12), (what, tag)
        assert close(g["centroid"][kg], w["centroid"][kw], 0.0 if exact else 1e-9, cen_abs), (what, tag)


def row_order(t, tag):
    """The order that aligns two tables: by (residue, voxels, density) -- the domain rows by (voxels, density)."""
    return np.lexsort((t["total"], t["n"], t["residue"] if tag == "res" else t["n"]))
