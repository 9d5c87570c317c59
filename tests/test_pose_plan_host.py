"""The host plan of pdbeda_pose_scores (pdb_eda_amd/csrc/pdbeda_poseplan.h) on a CPU: tests/pose_harness.cpp, built with the host compiler under
AddressSanitizer + UBSan (nothing recovered, nothing preloaded, nothing loaded into Python), run as one child process over one file of cases,
against the restatement in tests/pose_checker.py.  Every line is compared with ==.  It is the C++ that ships -- the header the library
includes -- not a copy.

Covered: every refusal of the argument check in its order; the reach and the centre refusals; the box of every centre of tests/pose_cases.py,
staged and with the global-only switch; the budget edge (31^3 and 32 x 32 x 31 staged, 32^3 and 33^3 not); the chunking on both sides of
its limit; the carve; and BRUTE FORCE: every voxel that any pose of a case's fragment touches -- under its own rotations and 2 000 more -- lies
in the centre's box, on the skewed cell as on the orthogonal ones."""
import os
import subprocess

import numpy as np
import pytest

from pdb_eda_amd import ccp4

import gradient_checker
import pose_cases as cases
import pose_checker as checker
import resample_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def text(v):
    return repr(float(v))


def flat(rows):
    return [text(v) for r in rows for v in r]


def build_cases():
    """[(record, expected line)]."""
    out = []

    def add_check(nf, nr, nc, top_k, flags, frag, w, rot, centres):
        record = ["check", nf, nr, nc, top_k, flags, len(w), len(rot) // 9, len(centres) // 3] + [text(v) for v in list(frag) + list(w) + list(rot) + list(centres)]
        refusal, at, radius = checker.check(nf, nr, nc, top_k, flags, frag, w, rot, centres)
        out.append((record, "check %d %d %.17g" % (refusal, at, radius if refusal in (checker.OK, checker.ROT_VALUE, checker.CENTRE_VALUE, checker.FRAG_VALUE) else 0.0)))

    frag, w = [0.5, 1.5, 2.5, -3.0, 4.0, 0.25], [1.0, -2.0]
    rot = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] * 2
    centres = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]
    add_check(2, 2, 3, 1, 0, frag, w, rot, centres)
    add_check(2, 2, 3, 64, 3, frag, w, rot, centres)
    add_check(2, 2, 0, 1, 0, frag, w, rot, [])
    for nf in (0, 257, -1):                                                                  # every refusal, in the order of the checks
        add_check(nf, 2, 3, 1, 0, [], [], rot, centres)
    for nr in (0, 2 ** 20 + 1, -1):
        add_check(2, nr, 3, 1, 0, frag, w, [], centres)
    for top_k in (0, 65, -1):
        add_check(2, 2, 3, top_k, 0, frag, w, rot, centres)
    for flags in (4, 0x80000001):
        add_check(2, 2, 3, 1, flags, frag, w, rot, centres)
    add_check(2, 2, -1, 1, 0, frag, w, rot, [])
    add_check(2, 2, 2 ** 31, 1, 0, frag, w, rot, [])
    add_check(2, 2, 2 ** 30, 1, 0, frag, w, rot, [])                                          # 2^30 * 2 = 2^31 poses
    add_check(2, 2 ** 20, 2 ** 11, 1, 0, frag, w, [], [])                                     # 2^31 poses exactly
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 5):
            add_check(2, 2, 3, 1, 0, frag[:at] + [bad] + frag[at + 1:], w, rot, centres)
        add_check(2, 2, 3, 1, 0, frag, [w[0], bad], rot, centres)
        add_check(2, 2, 3, 1, 0, frag, w, rot[:13] + [bad] + rot[14:], centres)
        add_check(2, 2, 3, 1, 0, frag, w, rot, centres[:7] + [bad] + centres[8:])
    add_check(0, 0, -1, 0, 4, [], [], [], [])                                                 # several at once: the first in the order
    add_check(2, 2, 3, 1, 0, [float("nan")] * 6, w, [float("nan")] * 18, [float("nan")] * 9)

    for case in cases.all_cases():
        rows, off, norm, _ = gradient_checker.grid_of(cases.header_of(case["map"]))
        radius = checker.radius_of(case["frag"])
        for c in case["centres"]:
            for global_only in (0, 1):
                lo, n, vox, staged = checker.box(rows, off, norm, [float(v) for v in c], radius, bool(global_only))
                out.append((["box"] + flat(rows) + [text(v) for v in off] + [text(v) for v in c] + [text(radius), global_only],
                            "box %d %d %d %d %d %d %d %d" % (tuple(lo) + tuple(n) + (vox, staged))))
    # the budget edge on a unit grid: 2 r + 1 + 4 voxels a side when the centre is on a voxel
    for c, radius in (([0.0, 0.0, 0.0], 13.0), ([0.5, 0.0, 0.0], 13.0), ([0.5, 0.5, 0.0], 13.0), ([0.5, 0.5, 0.5], 13.0), ([0.0, 0.0, 0.0], 13.5), ([0.5, 0.0, 0.0], 13.5), ([0.5, 0.5, 0.0], 13.5), ([0.5, 0.5, 0.5], 13.5), ([0.0, 0.0, 0.0], 14.0),
                      ([0.0, 0.0, 0.0], 0.0), ([-7.25, 1e6, 3.0], 2.0), ([0.0, 0.0, 0.0], 16382.0), ([0.0, 0.0, 0.0], 16383.0), ([2.0 ** 28, 0.0, 0.0], 2.0 ** 28)):
        lo, n, vox, staged = checker.box(UNIT, [0.0] * 3, [1.0] * 3, c, radius)
        out.append((["box"] + flat(UNIT) + ["0.0"] * 3 + [text(v) for v in c] + [text(radius), 0], "box %d %d %d %d %d %d %d %d" % (tuple(lo) + tuple(n) + (vox, staged))))

    for name in ("orth", "hex"):
        rows, off, _, _ = gradient_checker.grid_of(cases.header_of(name))
        for x in (0.0, 1e3, 2.0 ** 27, 2.0 ** 28, 2.0 ** 29, -2.0 ** 29, 1e300):
            out.append((["centre"] + flat(rows) + [text(v) for v in off] + [text(x), "0.0", "0.0"], "centre %d" % int(checker.centre_ok(rows, off, [x, 0.0, 0.0]))))
        for radius in (3.0, 2.0 ** 27, 2.0 ** 28, 2.0 ** 29, 1e300):
            out.append((["reach"] + flat(rows) + [text(radius)], "reach %d" % int(gradient_checker.reach_ok(gradient_checker.norms(rows), radius))))

    for nc, nr in ((0, 1), (1, 1), (3, 1), (500, 4096), (1260, 4096), (1261, 4096), (2000, 4096), (4, 2 ** 20), (5, 2 ** 20), (1, 2 ** 20), (2 ** 31 - 1, 1), (5162220, 1), (5162221, 1)):
        out.append((["chunk", nc, nr], "chunk %d" % checker.chunk(nc, nr)))
    for nf, nr, ch, top_k in ((1, 1, 1, 1), (256, 4096, 1260, 64), (20, 4096, 500, 5), (7, 257, 6, 5), (33, 2 ** 20, 4, 64)):
        out.append((["scratch", nf, nr, ch, top_k], "scratch %d" % checker.scratch_bytes(nf, nr, ch, top_k)))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("poseplan")
    exe, case_file = str(d / "pose_harness"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pose_harness.cpp"), "-o", exe])
    built = build_cases()
    with open(case_file, "w") as f:
        for record, _ in built:
            f.write(" ".join(str(x) for x in record) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return built, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    """No sanitizer report, and none of the invariants the harness asserts missed."""
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
    assert seen == {checker.OK, checker.ATOMS, checker.ROTATIONS, checker.TOP, checker.FLAG, checker.COUNT, checker.FRAG_VALUE, checker.ROT_VALUE, checker.CENTRE_VALUE}
    assert {w for r, w in built if r[0] == "reach"} == {"reach 0", "reach 1"} and {w for r, w in built if r[0] == "centre"} == {"centre 0", "centre 1"}


def test_the_budget_edge_and_the_chunk_limit():
    box = lambda c, r: checker.box(UNIT, [0.0] * 3, [1.0] * 3, c, r)
    assert box([0.0, 0.0, 0.0], 13.0)[1:] == ([31, 31, 31], 29791, 1)
    assert box([0.5, 0.0, 0.0], 13.0)[1:] == ([30, 31, 31], 28830, 1)                                  # (between voxels an integer radius spans one voxel less)
    assert box([0.5, 0.0, 0.0], 13.5)[1:] == ([32, 31, 31], 30752, 1) and box([0.5, 0.5, 0.0], 13.5)[1:] == ([32, 32, 31], 31744, 1)
    assert box([0.5, 0.5, 0.5], 13.5)[1:] == ([32, 32, 32], 32768, 0)                                  # 131 072 + 4 096 bytes: over by the stored bits
    assert box([0.0, 0.0, 0.0], 14.0)[1:] == ([33, 33, 33], 35937, 0)
    assert box([0.0, 0.0, 0.0], 0.0) == ([-2, -2, -2], [5, 5, 5], 125, 1)                              # every atom on the pivot: the support and the safety
    assert box([0.0, 0.0, 0.0], 16383.0)[2] == -1                                                      # a side beyond any budget: the product is not formed
    assert checker.box(UNIT, [0.0] * 3, [1.0] * 3, [0.0, 0.0, 0.0], 13.0, True)[3] == 0
    assert checker.lds_bytes(30752) == 123008 + 8 * 481 and checker.LDS_BUDGET == 128 * 1024 <= 160 * 1024
    assert checker.chunk(1260, 4096) == 1260 and checker.chunk(1261, 4096) == 1260 and checker.chunk(5162221, 1) == 5162220


@pytest.mark.parametrize("case", cases.all_cases(), ids=[c["tag"] for c in cases.all_cases()])
def test_the_box_holds_every_voxel_a_pose_touches(case):
    """The eight corners of every atom of every pose -- under the case's rotations and 2 000 lattice rotations more -- lie inside the plan's box of the
    centre: floor(f) >= lo and floor(f) + 1 <= lo + n - 1 on every axis, with f the device's grid position (tests/resample_checker.py)."""
    header = cases.header_of(case["map"])
    rot = np.concatenate([case["rot"].reshape(-1, 3, 3), ccp4.rotationLattice(2000)])
    frag = case["frag"]
    if len(frag) > 16:                                                                                # (the atoms farthest out decide; keep the test quick)
        far = np.argsort(-(frag * frag).sum(axis=1))[:16]
        frag = np.concatenate([frag[far], frag[:1] * 0.0 + frag[far[0]]])
    assert checker.radius_of(frag) == checker.radius_of(case["frag"])
    p = checker.positions(frag, rot, case["centres"])
    for ci, (lo, n, vox, staged) in enumerate(checker.boxes(header, case["frag"], case["centres"])):
        base = np.floor(resample_checker.xyz2frac(header, p[ci].reshape(-1, 3))).astype(np.int64)
        assert np.all(base >= np.array(lo)) and np.all(base + 1 <= np.array(lo) + np.array(n) - 1), (case["tag"], ci)
        assert np.all(base.min(axis=0) - np.array(lo) <= 3 + (0 if header.orthogonal else 2))          # (and the box is not idly large: at most the safety, and on the skewed cell the slack of the bound, to spare)
