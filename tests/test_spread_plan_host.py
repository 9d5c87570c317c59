"""The host plan of pdbeda_map_spread (pdb_eda_amd/csrc/pdbeda_spreadplan.h) on a CPU: tests/spread_harness.cpp, built with the host compiler under
AddressSanitizer + UBSan (nothing recovered, nothing preloaded, nothing loaded into Python), run as one child process over one file of cases,
against a restatement in Python.  Every line is compared with ==.  It is the C++ that ships -- the header the library includes -- not a copy.

Covered: the row-compilability of every table of tests/spread_cases.py with the expected verdict, the records and the rank array against the
restatement, the tile and the LDS at both ends of the reach, and every refusal of the argument check."""
import os
import subprocess

import numpy as np
import pytest

import spread_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_OFFSETS, MAX_REACH = 16384, 32
TILE_C, TILE_R, TILE_S = cases.TILE
LDS_TARGET, LDS_BUDGET = 40 * 1024, 128 * 1024
OK, COUNT, REACH, THRESHOLD, FLAG, AXIS, GRID = range(7)


def cdiv(a, b):
    return -((-a) // b)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def check(n, flags, nan, ncrs, interval, offsets):
    if n < 1 or n > MAX_OFFSETS:
        return [COUNT, 0, 0, 0]
    reach = [0, 0, 0]
    for o in offsets:
        for k in range(3):
            if abs(o[k]) > MAX_REACH:
                return [REACH] + reach
            reach[k] = max(reach[k], abs(o[k]))
    if nan:
        return [THRESHOLD] + reach
    if flags & ~1:
        return [FLAG] + reach
    if any(n_ <= 0 or n_ >= 2 ** 30 or i <= 0 for n_, i in zip(ncrs, interval)):
        return [AXIS] + reach
    return [OK] + reach


def plan(ncrs, reach, n_ranks):
    words = 2 if reach[0] > 0 else 1
    lds_ranks = cdiv(2 * n_ranks, 8) * 8
    bits = lambda tr, ts: 8 * words * (tr + 2 * reach[1]) * (ts + 2 * reach[2])
    tr, ts = TILE_R, TILE_S
    while bits(tr, ts) + lds_ranks > LDS_TARGET and (tr > 1 or ts > 1):
        if ts >= tr:
            ts //= 2
        else:
            tr //= 2
    box_r, box_s = tr + 2 * reach[1], ts + 2 * reach[2]
    tiles = [cdiv(ncrs[0], TILE_C), cdiv(ncrs[1], tr), cdiv(ncrs[2], ts)]
    n_tiles = tiles[0] * tiles[1] * tiles[2]
    return [GRID if n_tiles >= 2 ** 31 else OK, tr, ts, words, box_r, box_s, words * box_r * box_s, bits(tr, ts), lds_ranks, bits(tr, ts) + lds_ranks] + tiles + [n_tiles]


def compile_rows(offsets):
    """(ok, records [dr, ds, lo, len, m, best, start], ranks)."""
    groups = {}
    for t, (dc, dr, ds) in enumerate(offsets):
        groups.setdefault((int(ds), int(dr)), []).append((int(dc), t))
    records = []
    for (ds, dr), members in groups.items():
        members.sort()
        dcs, ts = [m[0] for m in members], [m[1] for m in members]
        if dcs != list(range(dcs[0], dcs[0] + len(dcs))):
            return False, [], []
        at = ts.index(min(ts))
        if any(ts[k] >= ts[k - 1] for k in range(1, at + 1)) or any(ts[k] <= ts[k - 1] for k in range(at + 1, len(ts))):
            return False, [], []
        if at > 64 or len(ts) - at > 64:
            return False, [], []
        records.append(([dr, ds, dcs[0], len(dcs), dcs[at], ts[at]], ts))
    records.sort(key=lambda r: r[0][5])
    rows, ranks = [], []
    for rec, ts in records:
        rows.append(rec + [len(ranks)])
        ranks += ts
    return True, rows, ranks


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def tables():
    """(tag, offsets, the verdict the table's maker expects)."""
    out = []
    for geometry in ("box", "skew", "rep"):
        for name in cases.TABLES:
            offsets, compilable = cases.table(name, geometry)
            out.append(("%s-%s" % (geometry, name), offsets, compilable))
    for geometry in ("box", "skew", "rep"):
        out.append(("%s-ball40" % geometry, cases.spreadTable(cases.header_of(geometry), 4.0)[0], True))
    out.append(("big-largest", cases.largest_ball()[0], True))
    two_minima = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0]], dtype=np.int32)             # ranks 0, 2, 1 along dc: a second minimum
    out.append(("two-minima", two_minima, False))
    out.append(("reversed-ball", cases.table("ball25", "box")[0][::-1], False))          # the middle rows rise to a maximum
    return out


def build_cases():
    """[(record, expected output lines)]."""
    out = []
    box, cell = [21, 9, 7], [21, 9, 7]
    ball = [list(map(int, o)) for o in cases.table("ball10", "box")[0]]
    flat = [v for o in ball for v in o]

    def add_check(n, flags, nan, ncrs, interval, offsets):
        record = ["check", n, flags, int(nan)] + ncrs + interval + [v for o in offsets for v in o]
        out.append((record, ["check " + " ".join(str(v) for v in check(n, flags, nan, ncrs, interval, offsets))]))

    add_check(len(ball), 0, False, box, cell, ball)
    add_check(len(ball), 1, False, box, [100, 9, 7], ball)
    add_check(0, 0, False, box, cell, [])                                                 # every refusal, in the order of the checks
    add_check(MAX_OFFSETS + 1, 0, False, box, cell, [])
    add_check(-3, 0, False, box, cell, [])
    add_check(MAX_OFFSETS, 0, False, box, cell, [[0, 0, 0]] * MAX_OFFSETS)                # the most that is taken
    for k in range(3):
        for v in (MAX_REACH + 1, -MAX_REACH - 1):
            far = [[0, 0, 0], [0, 0, 0]]
            far[1][k] = v
            add_check(2, 0, False, box, cell, far)
        edge = [[0, 0, 0], [0, 0, 0]]
        edge[0][k], edge[1][k] = MAX_REACH, -MAX_REACH
        add_check(2, 0, False, box, cell, edge)
    add_check(len(ball), 0, True, box, cell, ball)
    add_check(len(ball), 2, False, box, cell, ball)
    add_check(len(ball), 0x80000001, False, box, cell, ball)
    add_check(1, 0, False, [2 ** 30, 1, 1], [2 ** 30, 1, 1], [[0, 0, 0]])
    add_check(1, 0, False, [2 ** 30 - 1, 1, 1], [2 ** 30 - 1, 1, 1], [[0, 0, 0]])
    add_check(1, 0, False, [4, 0, 4], [4, 4, 4], [[0, 0, 0]])
    add_check(1, 0, False, [4, 4, 4], [4, 4, 0], [[0, 0, 0]])
    add_check(2, 3, True, box, cell, [[0, 0, 0], [0, 40, 0]])                             # several at once: the first in the order

    def add_plan(ncrs, reach, n_ranks):
        out.append((["plan"] + ncrs + reach + [n_ranks], ["plan " + " ".join(str(v) for v in plan(ncrs, reach, n_ranks))]))

    for reach in ([0, 0, 0], [1, 1, 1], [5, 5, 5], [8, 8, 8], [32, 0, 0], [0, 32, 0], [0, 0, 32], [16, 16, 16], [32, 32, 32], [3, 17, 9], [12, 11, 12], [12, 12, 12]):
        for n_ranks in (0, 1, 2145, MAX_OFFSETS):
            add_plan(box, reach, n_ranks)
    for ncrs in ([64, 8, 8], [65, 9, 9], [128, 16, 16], [1, 1, 1], [2 ** 30 - 1, 1, 1], [2 ** 30 - 1, 2 ** 10, 2 ** 10], [2 ** 20, 2 ** 20, 2 ** 10]):
        for reach in ([0, 0, 0], [8, 8, 8], [32, 32, 32]):
            add_plan(ncrs, reach, 100)

    for tag, offsets, _ in tables():
        ok, rows, ranks = compile_rows(offsets)
        lines = ["rows %d %d" % (int(ok), len(rows))] + ["row " + " ".join(str(v) for v in r) for r in rows] + [("ranks " + " ".join(str(v) for v in ranks)).rstrip()]
        out.append((["rows", len(offsets)] + [int(v) for v in np.asarray(offsets).reshape(-1)], lines))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("spreadplan")
    exe, case_file = str(d / "spread_harness"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "spread_harness.cpp"), "-o", exe])
    built = build_cases()
    with open(case_file, "w") as f:
        for record, _ in built:
            f.write(" ".join(str(x) for x in record) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return built, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    """No sanitizer report, and none of the invariants the harness asserts for accepted plans and compiled tables missed."""
    _, proc = run
    assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-2000:]


def test_every_line_agrees_with_the_restatement(run):
    built, proc = run
    got = proc.stdout.splitlines()
    want = [line for _, lines in built for line in lines]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.parametrize("entry", tables(), ids=lambda e: e[0])
def test_row_compilability_has_the_expected_verdict(entry):
    """Every ball of spreadTable is searched by rows (13 to 235 rows on these geometries at 1.0 to 4.0 A); a shuffled ball, a ball without a shell,
    a ball with a duplicate and a row of 65 rising ranks are walked."""
    tag, offsets, expected = entry
    ok, rows, ranks = compile_rows(offsets)
    assert ok == expected
    if ok:
        assert sorted(ranks) == list(range(len(offsets))) and [r[5] for r in rows] == sorted(r[5] for r in rows)
        if "ball" in tag and "largest" not in tag:
            assert 5 <= len(rows) <= 235


def test_the_budget_at_both_ends_of_the_reach():
    """No reach: the nominal tile and 512 B of bits.  The largest reach on every axis with the longest table: a tile of one row, 67 600 B of bits and
    32 KiB of ranks -- 100 368 B, inside the 128 KiB a workgroup is allowed (a CU has 160 KiB)."""
    small = plan([21, 9, 7], [0, 0, 0], 1)
    assert small[1:3] == [TILE_R, TILE_S] and small[3] == 1 and small[7] == 8 * TILE_R * TILE_S and small[9] == 8 * TILE_R * TILE_S + 8
    large = plan([21, 9, 7], [32, 32, 32], MAX_OFFSETS)
    assert large[1:3] == [1, 1] and large[3] == 2 and large[7] == 67600 and large[9] == 100368 <= LDS_BUDGET
    typical = plan([256, 256, 256], [8, 8, 8], 2109)
    assert typical[1:3] == [TILE_R, TILE_S] and typical[9] <= LDS_TARGET
