"""The host plan of pdbeda_atom_moments (pdb_eda_amd/csrc/pdbeda_gradplan.h) on a CPU: tests/gradient_harness.cpp, built with the host compiler
under AddressSanitizer + UBSan (nothing recovered, nothing preloaded, nothing loaded into Python), run as one child process over one file of
cases, against the restatement in tests/gradient_checker.py.  Every line is compared with ==.  It is the C++ that ships -- the header the
library includes -- not a copy.

Covered: every refusal of the argument check in its order, the reach and the 2^31-voxel refusals, the box of every atom of
tests/gradient_cases.py on every geometry, clipped to the stored and to the unique box, and against BRUTE FORCE: every voxel of the domain
that lies in a sphere lies in its box (on the skewed cell as on the orthogonal ones); S for zero, tiny and huge max|w| and on either side
of V_max = 2^22."""
import os
import subprocess

import numpy as np
import pytest

import gradient_cases as cases
import gradient_checker as checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(v):
    return repr(float(v))


def flat(rows):
    return [text(v) for r in rows for v in r]


def atom_boxes():
    """(geometry, unique, xyz, radius) of every atom the GPU test runs, and of the trips."""
    out = []
    for name in cases.GEOMETRIES:
        xyz, _, radii = cases.atoms(name, 1)
        for unique in (False, True):
            out += [(name, unique, [float(v) for v in p], float(r)) for p, r in zip(xyz, radii)]
    xyz, _, radii = cases.trips("wide")
    out += [("wide", False, [float(v) for v in p], float(r)) for p, r in zip(xyz, radii)]
    return out


def build_cases():
    """[(record, expected line)]."""
    out = []

    def add_check(n, nt, flags, xyz, expo, radii):
        given = len(radii)
        record = ["check", n, nt, flags, given] + [text(v) for v in xyz] + [text(v) for v in expo] + [text(v) for v in radii]
        refusal, at, top = checker.check(n, nt, flags, xyz, expo, radii)
        out.append((record, "check %d %d %.17g" % (refusal, at, top)))

    xyz, expo, radii = [0.5, 1.5, 2.5, 3.0, 4.0, 5.0], [1.0, 0.0, 2.0, 3.0], [float(np.float32(1.3)), float(np.float32(0.7))]
    add_check(2, 2, 0, xyz, expo, radii)
    add_check(2, 2, 1, xyz, expo, radii)
    add_check(0, 1, 0, [], [], [])
    for nt in (0, 7, -1):                                                                  # every refusal, in the order of the checks
        add_check(2, nt, 0, xyz, [], radii)
    add_check(2, 6, 0, xyz, expo * 3, radii)
    add_check(2, 2, 2, xyz, expo, radii)
    add_check(2, 2, 0x80000001, xyz, expo, radii)
    add_check(2 ** 31, 1, 0, [], [], [])
    add_check(-1, 1, 0, [], [], [])
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 4):
            add_check(2, 2, 0, xyz[:at] + [bad] + xyz[at + 1:], expo, radii)
        add_check(2, 2, 0, xyz, expo[:3] + [bad], radii)
        add_check(2, 2, 0, xyz, expo, [radii[0], bad])
    add_check(2, 2, 0, xyz, [1.0, -1e-300, 2.0, 3.0], radii)
    add_check(2, 2, 0, xyz, [1.0, -0.0, 2.0, 3.0], radii)                                   # (a negative zero is not negative)
    add_check(2, 2, 0, xyz, expo, [0.0, radii[1]])
    add_check(2, 2, 0, xyz, expo, [radii[0], -1.0])
    add_check(2, 7, 3, [float("nan")] * 6, [], radii)                                    # several at once: the first in the order

    for name, unique, p, r in atom_boxes():
        rows, off, norm, dom = checker.grid_of(cases.header_of(name), unique)
        lo, n, vox, clipped = checker.box(rows, off, norm, dom, p, r)
        out.append((["box"] + flat(rows) + [text(v) for v in off] + dom + [text(v) for v in p] + [text(r)],
                    "box %d %d %d %d %d %d %d %d %d" % (tuple(lo) + tuple(n) + (vox, int(clipped), 0))))
    unit = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for dom, p, r in (([2048, 2048, 512], [1000.0, 1000.0, 250.0], 5000.0),               # exactly 2^31 voxels: refused
                      ([2048, 2048, 511], [1000.0, 1000.0, 250.0], 5000.0),               # just below
                      ([2 ** 31 - 1, 1, 1], [5.0, 0.0, 0.0], 1e8),
                      ([10, 10, 10], [1e300, 0.0, 0.0], 1.0), ([10, 10, 10], [-1e300, 5.0, 5.0], 2.0),
                      ([10, 10, 10], [1.7976931348623157e308, 0.0, 0.0], 1.0)):
        scale = [[2.0 * v for v in row] for row in unit] if p[0] > 1e307 else unit         # (a grid position that overflows: an empty box)
        lo, n, vox, clipped = checker.box(scale, [0.0, 0.0, 0.0], checker.norms(scale), dom, p, r)
        out.append((["box"] + flat(scale) + ["0.0"] * 3 + dom + [text(v) for v in p] + [text(r)],
                    "box %d %d %d %d %d %d %d %d %d" % (tuple(lo) + tuple(n) + (vox, int(clipped), int(vox >= 2 ** 31)))))

    for name in ("box", "skew"):
        rows = checker.grid_of(cases.header_of(name))[0]
        for r_max in (3.0, 2.0 ** 27, 2.0 ** 28, 2.0 ** 29, 2.0 ** 31, 1e300):
            out.append((["reach"] + flat(rows) + [text(r_max)], "reach %d" % int(checker.reach_ok(checker.norms(rows), r_max))))

    for max_w in (0.0, 5e-324, 1e-300, 2.0 ** -30, 1.0, 3.0e6, 3.4e38, 1e250, float("inf"), float("nan")):
        for r_max in (0.2, 1.0, 3.0, 1e4):
            for v_max in (0, 27, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1, 2 ** 23, 2 ** 31 - 1):
                out.append((["shift", text(max_w), text(r_max), v_max], "shift %d" % checker.shift(max_w, r_max, v_max)))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("gradplan")
    exe, case_file = str(d / "gradient_harness"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gradient_harness.cpp"), "-o", exe])
    built = build_cases()
    with open(case_file, "w") as f:
        for record, _ in built:
            f.write(" ".join(str(x) for x in record) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return built, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    """No sanitizer report, and none of the invariants the harness asserts for every box missed."""
    _, proc = run
    assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-2000:]


def test_every_line_agrees_with_the_restatement(run):
    built, proc = run
    got = proc.stdout.splitlines()
    assert len(got) == len(built)
    for g, (_, w) in zip(got, built):
        assert g == w


def test_the_refusals_are_all_there(run):
    built, _ = run
    seen = {int(w.split()[1]) for r, w in built if r[0] == "check"}
    assert seen == {checker.OK, checker.TERMS, checker.FLAG, checker.COUNT, checker.XYZ, checker.EXPO, checker.RADIUS}
    assert {w for r, w in built if r[0] == "reach"} == {"reach 0", "reach 1"}
    large = [w.split() for r, w in built if r[0] == "box" and w.endswith(" 1")]
    assert len(large) == 1 and int(large[0][7]) == 2 ** 31


@pytest.mark.parametrize("name", cases.GEOMETRIES)
@pytest.mark.parametrize("unique", [False, True], ids=["stored", "unique"])
def test_the_box_covers_the_sphere_by_brute_force(name, unique):
    """Every voxel of the domain whose computed distance passes the contract's test lies inside the plan's box -- on the skewed cell, where the
    reference's box rule does not cover, as on the orthogonal ones; and the box stays inside the domain."""
    header = cases.header_of(name)
    rows, off, norm, dom = checker.grid_of(header, unique)
    crs = checker.domain_crs(header, unique)
    where = checker.voxel_xyz(header, crs, (name, unique))
    xyz, _, radii = cases.atoms(name, 1)
    extra = cases.trips("wide") if name == "wide" else None
    if extra is not None:
        xyz, radii = np.concatenate([xyz, extra[0]]), np.concatenate([radii, extra[2]])
    members = 0
    for p, r in zip(xyz, radii.astype(np.float64)):
        lo, n, vox, _ = checker.box(rows, off, norm, dom, [float(v) for v in p], float(r))
        dx, dy, dz = where[:, 0] - p[0], where[:, 1] - p[1], where[:, 2] - p[2]
        inside = np.sqrt((dx * dx + dy * dy) + dz * dz) <= r
        mine = crs[inside]
        members += len(mine)
        if len(mine):
            assert vox > 0 and np.all(mine >= np.array(lo)) and np.all(mine < np.array(lo) + np.array(n))
        assert all(0 <= lo[k] and lo[k] + n[k] <= dom[k] for k in range(3))
    assert members > 0


def test_the_trips_have_the_boxes_their_maker_says():
    header = cases.header_of("wide")
    rows, off, norm, dom = checker.grid_of(header)
    xyz, _, radii = cases.trips("wide")
    got = [tuple(checker.box(rows, off, norm, dom, [float(v) for v in p], float(r))[1]) for p, r in zip(xyz, radii)]
    assert got == cases.boxes_of_trips()


def test_shift_rule_at_its_edges():
    assert checker.shift(0.0, 3.0, 100) == 40 and checker.shift(float("nan"), 1.0, 1) == 40
    assert checker.shift(1.0, 1.0, 0) == 61 - 23 and checker.shift(1.0, 0.2, 2 ** 22) == 38          # B = 2^22 < 2^23
    assert checker.shift(1.0, 1.0, 2 ** 22 + 1) == 38 and checker.shift(1.0, 1.0, 2 ** 23 - 1) == 38 and checker.shift(1.0, 1.0, 2 ** 23) == 37
    assert checker.shift(1.0, 2.0, 27) == 36 and checker.shift(3.0e6, 1.0, 27) == 17 and checker.shift(0.999, 1.0, 27) == 39
    assert checker.shift(1e-300, 1.0, 27) == 900 and checker.shift(1e300, 1.0, 27) == -900          # (clamped: 1035 and -958)
