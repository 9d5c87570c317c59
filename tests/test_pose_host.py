"""CPU checks behind the pose-score tests: tests/pose_checker.py against a scalar brute force on tiny inputs (one pose, one atom, one corner at a
time, Python floats), the cases of tests/pose_cases.py against what their comments promise (so that no GPU test passes vacuously), and the
host helpers of pdb_eda_amd/ccp4.py: rotationLattice, rotationsNear, fragmentFrame, placeFragment."""
import math

import numpy as np
import pytest

from pdb_eda_amd import ccp4

import pose_cases as cases
import pose_checker as checker

_tables = {}


def table_of(case):
    if case["tag"] not in _tables:
        _tables[case["tag"]] = checker.scores(cases.header_of(case["map"]), cases.grid_of(case["map"]), case["frag"], case["w"], case["rot"], case["centres"],
                                              case["floor"], case["max_low"], case["allow_outside"])
    return _tables[case["tag"]]


# ---- the checker against brute force ----------------------------------------------------------------------------------------------------------
def brute_sample(header, grid, p):
    """One point, in Python floats: (value, valid)."""
    if header.orthogonal:
        q = [(p[i] - float(header.origin[i])) / float(header.gridLength[i]) for i in range(3)]
    else:
        fr = ccp4._dot3(np.asarray(header.deOrthoMat, dtype=np.float64), [float(v) for v in p])
        q = [float(fr[i]) * float(header.xyzInterval[i]) - float(header.crsStart[header.map2xyz[i]]) for i in range(3)]
    f = [q[header.map2crs[j]] for j in range(3)]
    if not all(abs(v) < 2.0 ** 29 for v in f):
        return float("nan"), False
    b = [math.floor(v) for v in f]
    t = [f[j] - b[j] for j in range(3)]
    v, valid = [], True
    for k in range(8):
        idx, stored = [], True
        for j, d in enumerate((k & 1, (k >> 1) & 1, k >> 2)):
            i, n, interval = b[j] + d, int(header.ncrs[j]), int(header.crsInterval[j])
            if i < 0 or i >= n:
                i %= interval
            stored = stored and not (n <= i < interval)
            idx.append(i)
        valid = valid and stored
        v.append(float(grid[idx[2], idx[1], idx[0]]) if stored else 0.0)
    lerp = lambda a, c, w: a + w * (c - a)
    c00, c10, c01, c11 = lerp(v[0], v[1], t[0]), lerp(v[2], v[3], t[0]), lerp(v[4], v[5], t[0]), lerp(v[6], v[7], t[0])
    return lerp(lerp(c00, c10, t[1]), lerp(c01, c11, t[1]), t[2]), valid


def brute(header, grid, frag, w, rot, centres, floor, max_low, allow):
    n, m = len(centres), len(rot)
    s, low, kept = np.zeros((n, m)), np.zeros((n, m), dtype=np.int32), np.zeros((n, m), dtype=bool)
    for ci, c in enumerate(centres):
        for ri, R in enumerate(rot):
            total, n_low, valid = 0.0, 0, True
            for a, x in enumerate(frag):
                p = [float(c[i]) + ccp4._fma(R[i][2], x[2], ccp4._fma(R[i][0], x[0], float(R[i][1]) * float(x[1]))) for i in range(3)]
                v, ok = brute_sample(header, grid, p)
                total = total + float(w[a]) * v
                n_low += 1 if v < float(np.float32(floor)) else 0
                valid = valid and ok
            s[ci, ri], low[ci, ri] = total, n_low
            kept[ci, ri] = not n_low > (2 ** 31 - 1 if max_low is None else max_low) and total == total and (valid or allow)
    return s, low, kept


@pytest.mark.parametrize("name", ["orth", "cut", "hex", "nan", "fine"])
def test_the_checker_agrees_with_brute_force(name):
    header, grid = cases.header_of(name), cases.grid_of(name)
    frag, w = cases.fragment(3, 1.2)
    rot = ccp4.rotationLattice(5)
    nc, nr, ns = (int(v) for v in header.ncrs)
    centres = np.array([cases.voxel(name, nc // 2, nr // 2, ns // 2), cases.voxel(name, nc - 1, nr - 1, ns - 1, (0.13, 0.07, -0.11)),
                        cases.voxel(name, cases.NAN_AT[2], cases.NAN_AT[1], cases.NAN_AT[0], (0.1, 0.1, 0.1)) if name == "nan" else cases.voxel(name, 1, 2, 3, (0.2, 0.1, 0.3))])
    for allow in (False, True):
        got = checker.scores(header, grid, frag, w, rot, centres, 0.0, 1, allow)
        s, low, kept = brute(header, grid, frag, w, rot, centres, 0.0, 1, allow)
        assert got["scores"].tobytes() == s.tobytes() or (np.array_equal(np.isnan(got["scores"]), np.isnan(s)) and np.array_equal(got["scores"][~np.isnan(s)], s[~np.isnan(s)]))
        assert np.array_equal(got["low"], low) and np.array_equal(got["kept"], kept)
    assert kept.any()


def test_on_a_voxel_centre_the_sample_is_the_voxel():
    """On the maps whose step is a power of two (0.5 A, origin 0) a voxel centre's grid position is an integer to the bit; the pivot case has such a centre."""
    for name in ("orth", "cube", "half"):
        header, grid = cases.header_of(name), cases.grid_of(name)
        v, ok = checker.sample(header, grid, cases.voxel(name, 5, 6, 7)[None, :])
        assert ok[0] and v[0] == float(grid[7, 6, 5])
    pivot = cases.find("pivot-3-64")
    assert np.array_equal(pivot["centres"][-1], cases.voxel("orth", 7, 9, 11))
    rho = float(cases.grid_of("orth")[11, 9, 7])
    assert np.all(table_of(pivot)["scores"][-1] == (1.0 * rho + 2.0 * rho) + 3.0 * rho)


def test_ranking_breaks_ties_by_index_and_treats_zeros_as_equal():
    table = {"scores": np.array([[1.0, -0.0, 0.0, 1.0, np.nan, np.inf]]), "low": np.arange(6, dtype=np.int32)[None, :], "kept": np.array([[True, True, True, True, False, True]])}
    rot, score, low, n = checker.ranking(table, 7)
    assert rot.tolist() == [[5, 0, 3, 1, 2, -1, -1]] and n.tolist() == [5] and low.tolist() == [[5, 0, 3, 1, 2, 0, 0]]
    assert score[0, 5:].tobytes() == np.zeros(2).tobytes() and np.signbit(score[0, 3]) and not np.signbit(score[0, 4])


# ---- the cases hold what they promise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.all_cases(), ids=[c["tag"] for c in cases.all_cases()])
def test_no_case_is_vacuous(case):
    table = table_of(case)
    kept = table["kept"]
    if case["ranked"]:
        assert kept.any(axis=1).any() and (~kept).any(axis=1).any(), "a ranked case needs a centre with kept poses and a centre with a rejected pose"
    assert 1 <= len(case["frag"]) <= checker.MAX_ATOMS and 1 <= case["top_k"] <= checker.MAX_TOP
    header = cases.header_of(case["map"])
    assert all(24 <= int(v) <= 32 for v in header.ncrs) or case["map"] in ("cut", "perm", "fine")


def test_the_cases_cover_the_sizes_and_paths_the_issue_names():
    all_cases = cases.all_cases()
    assert {len(c["frag"]) for c in all_cases} >= {1, 2, 7, 64, 65, checker.MAX_ATOMS}
    assert {len(c["rot"]) for c in all_cases} >= {1, 63, 64, 65, 257}
    assert {c["top_k"] for c in all_cases} >= {1, checker.MAX_TOP}
    fits, exceeds, fine = cases.find("stage-fits"), cases.find("stage-exceeds"), cases.find("fine-wraps")
    for c, staged, side in ((fits, 1, 31), (exceeds, 0, 33)):
        for lo, n, vox, st in checker.boxes(cases.header_of(c["map"]), c["frag"], c["centres"]):
            assert n == [side] * 3 and st == staged and vox == side ** 3
    assert checker.lds_bytes(31 ** 3) <= checker.LDS_BUDGET < checker.lds_bytes(32 ** 3)
    assert abs(checker.radius_of(exceeds["frag"]) - checker.radius_of(fits["frag"])) == 0.5              # one voxel of 0.5 A
    for lo, n, vox, st in checker.boxes(cases.header_of("fine"), fine["frag"], fine["centres"]):
        assert st == 1 and all(v > 3 * 8 for v in n)                                                     # wider than three cells of 8 voxels


def test_the_crafted_centres_do_what_their_comments_say():
    cut, outside = table_of(cases.find("cut-7-65")), table_of(cases.find("cut-7-65-outside"))
    assert not cut["valid"][2].all() and not cut["kept"][2].all() and cut["kept"][:2].any()            # the last stored voxel: atoms outside
    assert outside["kept"][2].sum() > cut["kept"][2].sum() and cut["scores"].tobytes() == outside["scores"].tobytes()
    half = table_of(cases.find("half-low"))
    assert half["kept"][0].all() and not half["kept"][1].any()                                          # none rejected / every pose rejected
    nan = table_of(cases.find("nan-7-64"))
    assert np.isnan(nan["scores"][0]).any() and not nan["kept"][0].all() and nan["kept"][2].all() and np.isinf(nan["scores"][1]).any()
    pivot = table_of(cases.find("pivot-3-64"))
    assert all(len(set(row.tolist())) == 1 for row in pivot["scores"])                                  # every rotation ties
    centro = table_of(cases.find("centro-8-7"))
    assert centro["scores"][:, 0].tobytes() == centro["scores"][:, 1].tobytes() and centro["kept"].all()
    few = cases.find("orth-1-1")
    assert few["top_k"] > len(few["rot"])
    far = cases.find("orth-7-257")["centres"][1]
    f = checker.resample_checker.xyz2frac(cases.header_of("orth"), far[None, :])[0]
    assert f[0] > 4 * 24 and f[1] < -2 * 26 and table_of(cases.find("orth-7-257"))["valid"][1].all()     # far outside a repeating map: it wraps


# ---- the host helpers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64, 257, 4096])
def test_rotation_lattice_is_orthonormal_and_deterministic(n):
    R = ccp4.rotationLattice(n)
    assert R.shape == (n, 3, 3) and R.dtype == np.float64
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() <= 1e-14
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-14
    assert ccp4.rotationLattice(n).tobytes() == R.tobytes()


def test_rotation_lattice_is_near_uniform():
    """No rotation of a 4096 lattice is farther from its nearest neighbour than 2.5 times the median such distance, and none is a duplicate."""
    R = ccp4.rotationLattice(4096)
    trace = np.einsum("aij,bij->ab", R[:512], R)
    angle = np.arccos(np.clip(0.5 * (trace - 1.0), -1.0, 1.0))
    angle[np.arange(512), np.arange(512)] = np.inf
    nearest = angle.min(axis=1)
    assert nearest.min() > 0.02 and nearest.max() < 2.5 * np.median(nearest)


def test_rotations_near_stay_within_their_angle():
    base = ccp4.rotationLattice(9)[4]
    for angle, n in ((0.5, 1), (0.5, 2), (0.3, 257), (1e-3, 64)):
        near = ccp4.rotationsNear(base, angle, n)
        assert near.shape == (n, 3, 3) and near[0].tobytes() == base.tobytes()
        assert ccp4.rotationAngle(near, base).max() <= angle * (1.0 + 1e-9) + 1e-7      # (arccos near 1 resolves 1e-8)
        assert np.abs(np.einsum("nij,nkj->nik", near, near) - np.eye(3)).max() <= 1e-14
        assert ccp4.rotationsNear(base, angle, n).tobytes() == near.tobytes()
    assert ccp4.rotationAngle(ccp4.rotationsNear(base, 0.3, 257), base).max() > 0.29     # the angle is used up


def test_fragment_frame():
    xyz = np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [1.0, 4.0, 3.0]])
    frame = ccp4.fragmentFrame(xyz, [1.0, 1.0, 2.0])
    assert np.allclose(frame["centroid"], [1.25, 3.0, 3.0]) and np.allclose(frame["xyz"] + frame["centroid"], xyz)
    assert frame["radius"] == checker.radius_of(frame["xyz"])
    plain = ccp4.fragmentFrame(xyz)
    assert np.allclose(plain["centroid"], xyz.mean(axis=0)) and np.all(plain["weights"] == 1.0)
    assert np.allclose(ccp4.fragmentFrame(xyz, [1.0, -1.0, 0.0])["centroid"], xyz.mean(axis=0))      # weights that sum to zero
    with pytest.raises(ValueError):
        ccp4.fragmentFrame(xyz, [1.0])


def test_place_fragment_equals_the_checkers_positions_to_the_bit():
    frag, w = cases.fragment(65)
    rot = ccp4.rotationLattice(7)
    centres = cases.interior("hex", 3)
    want = checker.positions(frag, rot, centres)
    frame = ccp4.fragmentFrame(frag + 5.0, w)
    for c in range(3):
        for r in range(7):
            assert ccp4.placeFragment(frag, centres[c], rot[r]).tobytes() == want[c, r].tobytes()
    assert ccp4.placeFragment(frame, centres[0], rot[0]).shape == (65, 3)
    assert np.allclose(ccp4.placeFragment(frag, [0.0, 0.0, 0.0], np.eye(3)), frag)


def test_plan_restatement_of_the_chunks_and_the_carve():
    assert checker.chunk(500, 4096) == 500 and checker.chunk(2000, 4096) == 1260 and checker.chunk(5, 2 ** 20) == 4 and checker.chunk(3, 1) == 3
    assert checker.chunk(1, 2 ** 20) == 1 and (64 << 20) // (13 * 2 ** 20) == 4
    assert checker.scratch_bytes(1, 1, 1, 1) == 12 * 256
