"""The inputs of tests/test_gpu_voxelsets.py pinned without a GPU, with the oracle and numpy alone: what the seeded lists, sets, atoms and
operators of tests/voxelsets_cases.py contain (so that the GPU test cannot pass because an input lost the property it was made for),
the conditioning of the blobs whose centroids it compares, the host fold of DeviceMap.list_stats restated over the oracle's components,
and the ties of the nearest-atom cases."""
import numpy as np
import pytest

import voxelsets_cases as cases


@pytest.fixture(scope="module", params=cases.WORLDS)
def world(request):
    from oracle import oracle as ora
    w = cases.world(request.param)
    return w, ora.Oracle(w.header, w.grid), cases.list_groups(request.param)


def unique_rows(vox):
    return np.unique(np.asarray(vox, dtype=np.int32).reshape(-1, 3), axis=0)


def test_point_density_of_the_cases_is_the_oracles(world):
    """cases.density (numpy) chooses every voxel of the lists: the oracle's getPointDensityFromCrs on a sample of them, and on the point rows."""
    w, o, full = world
    rows = np.concatenate([full.crs[::97], cases.point_rows(w.name)[::7]])
    assert np.array_equal(cases.density(w, rows), np.array([o.point_density(v) for v in rows]))
    valid = np.array([o.valid_crs(v) for v in cases.point_rows(w.name)])
    assert valid.any() and (w.name == "orth" or not valid.all())


def test_list_groups_hold_what_they_were_made_for(world):
    w, o, full = world
    sizes = np.diff(full.off)
    kinds = set(full.kind)
    assert {"a", "b", "c63", "c64", "c65", "c130", "d", "e", "f", "g"} <= kinds and (w.name == "orth" or "z" in kinds)
    assert np.array_equal(full.off, np.concatenate([[0], np.cumsum([len(g) for g in full.groups])])) and full.off[-1] == len(full.crs)
    # sizes: beyond one staged row of voxels; the head below it; the middle list between the voxels' limit and the group ids'
    variants = cases.list_variants(w.name)
    assert len(full.crs) * cases.LIST_ROW > cases.STAGED_ROW and len(full.crs) * 4 > cases.STAGED_ROW
    assert 2000 < len(variants["head"].crs) < cases.STAGED_ROW // cases.LIST_ROW == 21845
    assert cases.STAGED_ROW // cases.LIST_ROW < len(variants["middle"].crs) < cases.STAGED_ROW // 4
    # empty groups: the first, the last, runs, at least 100 in all
    assert sizes[0] == 0 and sizes[-1] == 0 and np.count_nonzero(sizes == 0) >= 100
    runs = np.flatnonzero((sizes[:-2] == 0) & (sizes[1:-1] == 0) & (sizes[2:] == 0))
    assert len(runs) >= 3
    # with four voxels a thread in k_list_boxes: group boundaries inside shares
    inner = full.off[1:-1]
    assert np.count_nonzero(inner % 4 != 0) >= 100
    assert np.count_nonzero((inner // 64 == (inner - 1) // 64) & (inner % 4 != 0)) >= 100          # ... and inside a wave's 256 voxels
    # (a) 0 to 9 voxels, reaching outside the stored grid on both sides of every axis
    small = [full.groups[g] for g in range(len(sizes)) if full.kind[g] == "a"]
    assert len(small) == cases.SMALL_GROUPS and max(len(g) for g in small) == 9 and min(len(g) for g in small) == 0
    every = np.concatenate(small)
    for k in range(3):          # (a voxel above the cutoff is a stored one: where part of the cell is not stored -- skew's rows -- the whole boxes of (g) reach outside)
        assert every[:, k].min() >= -6 and every[:, k].max() < w.ncrs[k] + 6
        assert (every[:, k].min() < 0 and every[:, k].max() >= w.ncrs[k]) or w.interval[k] > w.ncrs[k]
        assert full.crs[:, k].min() < 0 and full.crs[:, k].max() >= w.ncrs[k]
    # (b) about 10^5 voxels in one group, between small groups: whole waves and blocks of k_list_boxes hold one group
    b = full.kind.index("b")
    assert 8e4 < sizes[b] < 1.3e5 and full.kind[b - 2] == "a" and full.kind[b + 1] == "a"
    # (c) bounding boxes exactly 63, 64, 65 and 130 voxels wide in c
    for width in cases.WIDTHS:
        vox = full.groups[full.kind.index("c%d" % width)]
        assert vox[:, 0].max() - vox[:, 0].min() + 1 == width
    # (d) duplicates that np.unique removes; (e) one set in two groups, in two orders
    for g in (g for g in range(len(sizes)) if full.kind[g] == "d"):
        assert len(unique_rows(full.groups[g])) * 4 // 3 == len(full.groups[g]) > len(unique_rows(full.groups[g])) >= 6
    e1, e2 = (g for g in range(len(sizes)) if full.kind[g] == "e")
    assert e2 - e1 > 1000 and not np.array_equal(full.groups[e1], full.groups[e2]) and np.array_equal(unique_rows(full.groups[e1]), unique_rows(full.groups[e2]))
    # (f) periodic images: two voxels an interval apart, the same stored density, two blobs
    images = [full.groups[g] for g in range(len(sizes)) if full.kind[g] == "f"]
    assert len(images) == 3
    for k, vox in enumerate(images):
        step = np.abs(vox[1].astype(np.int64) - vox[0])
        assert step[k] == w.interval[k] and step.sum() == w.interval[k]
        rho = cases.density(w, vox)
        assert rho[0] == rho[1] != 0.0 and len(o.cluster(vox)) == 2
    # (g) whole boxes, whatever their density; in skew some hold unstored voxels (density 0), and "z" holds nothing else
    free = [full.groups[g] for g in range(len(sizes)) if full.kind[g] == "g"]
    assert all(len(vox) == 36 and len(o.cluster(vox)) == 1 for vox in free)
    mixed = sum(1 for vox in free if (cases.density(w, vox) > 0).any() and (cases.density(w, vox) < 0).any())
    assert mixed >= 4
    if w.name == "skew":
        assert sum(1 for vox in free if not all(o.valid_crs(v) for v in vox) and any(o.valid_crs(v) for v in vox)) >= 2
        zero = full.groups[full.kind.index("z")]
        assert len(zero) >= 12 and not any(o.valid_crs(v) for v in zero) and o.blob_stats(zero)["totalDensity"] == 0.0
    # extents the oracle's clustering grid can hold; three quarters of the groups of one sign
    one_sign = 0
    for vox in full.groups:
        if len(vox):
            assert (vox.max(axis=0).astype(np.int64) - vox.min(axis=0) + 1).max() <= 200
            rho = cases.density(w, vox)
            one_sign += bool((rho > w.cut).all() or (rho < -w.cut).all())
    assert one_sign >= 0.75 * np.count_nonzero(sizes)


def test_blobs_of_the_list_are_many_and_well_conditioned(world):
    """At least 30 % of the non-empty groups fall apart into two or more blobs, and fewer than 10 % of all blobs have |totalDensity| <
    0.01 sum |rho| -- those have an ill-conditioned density-weighted centroid, which tests/test_gpu_voxelsets.py leaves out of its
    centroid comparison (thresholded groups gave none at all; the whole boxes of (g) are the only possible source)."""
    w, o, full = world
    multi = nonempty = blobs = ill = 0
    for vox in full.groups:
        if not len(vox):
            continue
        found = o.blob_list(unique_rows(vox))
        nonempty += 1
        multi += len(found) >= 2
        assert sum(len(b["crs"]) for b in found) == len(unique_rows(vox))
        for b in found:
            blobs += 1
            ill += bool(abs(b["totalDensity"]) < 0.01 * np.abs(cases.density(w, b["crs"])).sum())
    print("%s: %d non-empty groups, %d of two or more blobs; %d blobs, %d ill-conditioned" % (w.name, nonempty, multi, blobs, ill))
    assert multi >= 0.3 * nonempty
    assert ill < 0.1 * blobs


def fold(rows):
    """DeviceMap.list_stats restated: the statistics of a voxel set from those of its connected components (dicts of Oracle.blob_stats)."""
    n = np.array([r["n"] for r in rows], dtype=np.float64)
    total = np.array([r["totalDensity"] for r in rows])
    has = total != 0          # (a component of total density 0 has no centroid of its own, 0 / 0, and adds nothing to the weighted sum)
    tot = float(total.sum())
    centroid = sum(np.asarray(r["centroid"]) * r["totalDensity"] for r, h in zip(rows, has) if h) / tot
    centre = sum(np.asarray(r["coordCenter"]) * r["n"] for r in rows) / n.sum()
    return {"totalDensity": tot, "centroid": centroid, "coordCenter": centre, "volume": float(sum(r["volume"] for r in rows)), "n": int(n.sum())}


def test_list_stats_fold_over_the_oracles_components(world):
    """What the GPU test demands of list_stats: the fold of the components' rows IS the reference's blob over the whole set (rtol 1e-12: both
    are fp64 sums of the same terms in another order; the sets are of one sign per part, so nothing cancels inside a part)."""
    w, o, full = world
    sets = cases.fold_sets(w.name)
    assert [s[0] for s in sets][:3] == ["pair0", "pair1", "pair2"] and (w.name == "orth" or sets[-1][0] == "zero")
    picked = [g for g in range(len(full.groups)) if full.kind[g] in ("a", "d") and len(full.groups[g]) >= 4][:200]
    tested = 0
    for label, vox in [(s[0], np.concatenate([s[1], s[2]])) for s in sets] + [("group %d" % g, full.groups[g]) for g in picked]:
        vox = unique_rows(vox)
        parts = o.blob_list(vox)
        if label.startswith("group") and len(parts) < 2:
            continue
        assert len(parts) >= 2, label
        if label == "zero":
            assert sum(1 for p in parts if p["totalDensity"] == 0.0) == 1 and all(np.isnan(p["centroid"]).all() for p in parts if p["totalDensity"] == 0.0)
        got, want = fold(parts), o.blob_stats(vox)
        assert got["n"] == want["n"] == len(vox)
        for k in ("totalDensity", "volume", "centroid", "coordCenter"):
            assert np.allclose(got[k], want[k], rtol=1e-12, atol=0), (label, k, got[k], want[k])
        tested += 1
    assert tested >= 50
    # the parts of a pair are disjoint and not adjacent
    from oracle import oracle as ora
    for label, a, b in sets:
        assert not ora.test_overlap(a, b), label


def test_overlap_sets_decide_at_the_last_pair():
    from oracle import oracle as ora
    s = cases.overlap_sets()
    assert sorted(set(len(v) for v in s.sets)) == [0, 1, 255, 256, 257, 1500]
    assert s.crs.min() < 0 and all(len(np.unique(v, axis=0)) == len(v) for v in s.sets if len(v))
    seen = {"touch": 0, "miss": 0}
    for a, b, what in s.pairs:
        A, B = s.sets[a], s.sets[b]
        want = ora.test_overlap(A, B)
        if what.startswith("touch"):
            d = np.abs(A[:, None, :] - B[None, :, :]).max(axis=2)
            assert want and np.argwhere(d <= 1).tolist() == [[len(A) - 1, len(B) - 1]], what
            seen["touch"] += 1
        elif what.startswith("miss"):
            d = np.sort(np.abs(A[-1] - B[-1]))
            assert not want and d.tolist() == [0, 0, 2], what
            seen["miss"] += 1
        elif "empty" in what:
            assert not want
        elif "itself" in what:
            assert want and a == b
        else:
            assert not want
    assert seen == {"touch": 14, "miss": 4}


def test_nearest_cases_really_tie():
    """scipy's cdist gives the tied atoms bit-equal distances, the minimum of their rows; np.argmin then returns the lower index."""
    from scipy.spatial.distance import cdist
    found = {}
    for case in cases.nearest_cases():
        n = len(case.atoms)
        d = cdist(case.centroids, case.atoms)
        first = np.argmin(d, axis=1)
        for row, lo, hi, what in case.ties:
            assert lo < hi < n and d[row, lo] == d[row, hi] == d[row].min() and first[row] == lo, (n, what)
            assert np.count_nonzero(d[row] == d[row].min()) == 2 and (("on a dup" in what or "middle" in what) or d[row, lo] > 0), (n, what)
            found.setdefault(n, set()).add((hi - lo, d[row, lo] == 0.0, np.array_equal(case.atoms[lo], case.atoms[hi])))
        assert len(np.unique(case.atoms, axis=0)) == n - sum(1 for t in {t[1:3] for t in case.ties} if np.array_equal(case.atoms[t[0]], case.atoms[t[1]]))
    assert [len(c.atoms) for c in cases.nearest_cases()] == list(cases.ATOM_COUNTS) and 24 * cases.ATOM_COUNTS[-1] > cases.STAGED_ROW
    assert 1 not in found
    gaps = {n: {g for g, _, _ in rows} for n, rows in found.items()}
    assert gaps[255] == gaps[256] == {1, 7} and gaps[257] == {1, 7, 256} and gaps[1000] == {1, 7, 256, 515} and gaps[12000] == {1, 7, 256, 10243}
    for n, rows in found.items():          # a tie at distance 0, ties of duplicates at a distance, ties of distinct atoms
        assert any(zero for _, zero, _ in rows) and any(same and not zero for _, zero, same in rows) and any(not same for _, _, same in rows)
    sizes = cases.nearest_batch_sizes()
    assert sizes == (262144, 262145, 524288, 524289)


def test_symmetry_cases_against_the_oracle():
    from oracle import oracle as ora
    kept = {}
    for label, xyz, rot, ortho, lo, hi in cases.symmetry_cases():
        total = 27 * len(rot) * len(xyz)
        idx, sym, out = ora.symmetry_atoms(xyz, rot, ortho, lo, hi)
        kept[label] = (len(idx), total)
        if label != "huge":
            assert total % 64 != 0 and total % 256 != 0
        assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)
    assert [len(c[2]) for c in cases.symmetry_cases()] == [1, 2, 4, 4, 4]
    assert kept["huge"] == (216000, 216000) and 8 * 216000 <= cases.PINNED_BLOCK < 24 * 216000
    assert kept["tight"][0] < 0.05 * kept["tight"][1] and kept["tight"][0] > 333          # most images dropped, some beyond the identity kept
    for label in ("one", "two", "four"):
        assert len(cases.symmetry_atoms_xyz(1)) == 1 and kept[label][1] // 27 < kept[label][0] < kept[label][1]


def test_point_batch_sizes_follow_from_the_bytes_per_row():
    span = cases.pinned_span
    for in_bytes, out_bytes in ((12, 8), (12, 1), (12, 24), (24, 12)):
        sizes = cases.point_batch_sizes(in_bytes, out_bytes)
        both = sizes[0]
        assert span(in_bytes * both) + span(out_bytes * both) <= cases.PINNED_BLOCK < span(in_bytes * (both + 1)) + span(out_bytes * (both + 1))
        assert sizes[1] == both + 1 and span(in_bytes * sizes[1]) <= cases.PINNED_BLOCK
        assert in_bytes * sizes[-1] > cases.PINNED_BLOCK and out_bytes * sizes[-1] > cases.PINNED_BLOCK
        assert any(in_bytes * n <= cases.PINNED_BLOCK < in_bytes * (n + 1) for n in sizes)
    assert cases.point_batch_sizes(12, 8) == [209712, 209713, 349525, 349526, 524289]          # (209 712: the last count whose two takes, in whole lines, fit)
