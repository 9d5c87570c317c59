"""The host's planner of labelling jobs and of the integer sums' quantum (pdb_eda_amd/csrc/pdbeda_jobplan.h) on a CPU: tests/jobplan_harness.cpp,
built with the host compiler under AddressSanitizer + UBSan and -ffp-contract=off (nothing recovered, nothing preloaded, nothing loaded into
Python), run as one child process over one file of cases, against a restatement in Python integers (math.frexp / math.ldexp for the quantum).
Every line is compared with ==.  It is the C++ that ships -- the header the library includes -- not a copy of it.

What no GPU test can afford is reached here: the three "grid too large" refusals of a whole-map job (1107^3 fused, 1281^3 single, 524 281
voxels along r or s, 2^31 keys), the switch of the rank counters' groups from 16 to 32 at 2^25 keys (256^3 fused: which k_labels_tiles
instantiation runs), and the quantum's shift at the ends of fp64.  For every accepted plan and every key table the harness itself asserts what
the kernels and the host's casts rely on (ids below 2^31, at most KEY_GROUPS groups, whole groups of counters, clears that cover their tables,
group totals exactly where they are summed); a miss, like a sanitizer report, ends it with a non-zero status."""
import math
import os
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_R = TILE_S = 8
TILE_COMPS, KEY_FINE, KEY_GROUPS = 256, 32, 1024
TILES_EMPTY, TILES_2P31, TILES_AXIS = 1, 2, 4
PLAN_OK, PLAN_KEYS, PLAN_AXIS, PLAN_RUN_IDS = 0, 1, 2, 3
FLT_MAX = float.fromhex("0x1.fffffep127")
INF, NAN = float("inf"), float("nan")


def cdiv(a, b):
    return -((-a) // b)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def tile_grid(d, tc, tr, ts):
    nc, nr, ns = cdiv(d[0], tc), cdiv(d[1], tr), cdiv(d[2], ts)
    n = nc * nr * ns
    return nc, nr, ns, n, (TILES_EMPTY if min(d) <= 0 else 0) | (TILES_2P31 if n >= 2 ** 31 else 0) | (TILES_AXIS if max(nr, ns) > 65535 else 0)


PLAN_FIELDS = ("refusal", "row_words", "ctiles", "cw", "rtiles", "stiles", "tiles_pp", "words_pp", "keys_pp", "total_words", "total_keys", "worst_blobs",
               "tile_runs", "tile_comps", "worst_unit", "run_ids_needed", "unit_ids", "max_runs", "max_comps", "max_blobs", "lab_elems")


def plan_whole_map(uc, ur, us, planes, worst, labels):
    p = dict.fromkeys(PLAN_FIELDS, 0)
    half = lambda n: (n + 1) // 2
    p["row_words"] = cdiv(uc, 64)
    p["words_pp"], p["keys_pp"] = p["row_words"] * ur * us, uc * ur * us
    p["total_words"], p["total_keys"] = p["words_pp"] * planes, p["keys_pp"] * planes
    p["worst_blobs"] = half(uc) * half(ur) * half(us) * planes + 1          # a blob per aligned 2x2x2 cell
    p["lab_elems"] = p["keys_pp"] if labels else 0
    p["ctiles"] = cdiv(p["row_words"], 4)
    p["cw"] = cdiv(p["row_words"], p["ctiles"])                             # equal widths: 5 words are 3 + 2
    p["rtiles"], p["stiles"] = cdiv(ur, TILE_R), cdiv(us, TILE_S)
    p["tiles_pp"] = p["ctiles"] * p["rtiles"] * p["stiles"]
    if p["tiles_pp"] >= 2 ** 31 or p["keys_pp"] >= 2 ** 31:
        return dict(p, refusal=PLAN_KEYS)
    if p["rtiles"] > 65535 or p["stiles"] > 65535:
        return dict(p, refusal=PLAN_AXIS)
    p["tile_runs"], p["tile_comps"] = p["tiles_pp"] * p["cw"] * 64 * 32, p["tiles_pp"] * TILE_COMPS
    p["worst_unit"] = half(uc) * ur * us * planes + 1                        # every other voxel a run
    p["run_ids_needed"] = p["tile_runs"] + p["worst_unit"]
    if p["run_ids_needed"] >= 2 ** 31:
        return dict(p, refusal=PLAN_RUN_IDS)
    p["unit_ids"] = p["worst_unit"] if worst else min(p["worst_unit"], max(65536, p["tile_runs"] // 4))
    p["max_blobs"] = p["worst_blobs"] if worst else min(p["worst_blobs"], max(4096, p["total_keys"] // 32))
    p["max_runs"], p["max_comps"] = p["tile_runs"] + p["unit_ids"], p["tile_comps"] + p["unit_ids"]
    return p


KEY_FIELDS = ("key_words", "n_fine", "fine_shift", "fine_per_group", "n_groups", "n_fine_alloc", "key_bits", "fine_count", "mid_count", "has_group_count",
              "clear_bits", "clear_fine", "clear_mid")


def plan_key_table(total_keys, n_tiles):
    k = dict.fromkeys(KEY_FIELDS, 0)
    k["key_words"] = cdiv(total_keys, 64)
    k["n_fine"] = buckets = cdiv(k["key_words"], KEY_FINE)
    shift = 4
    while (KEY_GROUPS << shift) < buckets:
        shift += 1
    k["fine_shift"], k["fine_per_group"] = shift, 1 << shift
    k["n_groups"] = cdiv(buckets, 1 << shift)
    k["n_fine_alloc"] = k["n_groups"] << shift
    k["key_bits"], k["fine_count"], k["mid_count"] = buckets * KEY_FINE, max(k["n_fine_alloc"] // 2, 8), buckets * (KEY_FINE // 16)
    k["has_group_count"] = 1 if n_tiles and shift > 4 else 0
    if n_tiles:
        k["clear_bits"], k["clear_fine"], k["clear_mid"] = cdiv(k["key_words"], n_tiles), cdiv(k["n_fine_alloc"] // 2, n_tiles), cdiv(k["mid_count"], n_tiles)
    return k


def quantum_shift(bound):
    S = 40
    if bound > 0.0 and math.isfinite(bound):
        S = 61 - math.frexp(bound)[1]          # bound < 2^e
    return max(-900, min(S, 900))


def map_quantum(sum_abs, max_abs):
    if not (math.isfinite(sum_abs) and math.isfinite(max_abs)):
        return 1, 0.0
    return 0, math.ldexp(1.0, quantum_shift(max(sum_abs, 4194304.0 * max_abs)))


def box_quantum(max_abs, n_vox):
    return math.ldexp(1.0, quantum_shift(max_abs * float(max(n_vox, 2 ** 22))))


def halvings(largest):
    h, room = 0, 2 ** 22
    while room < largest:
        h, room = h + 1, room * 2
    return h


def model_shift(n_gridded, a_max):
    prod = float(n_gridded) * a_max
    S = 40
    if not prod > 0.0:
        return S
    while S > -1000 and ldexp(prod, S) > 2.0 ** 62:
        S -= 1
    return S


def ldexp(x, e):
    """C's ldexp: infinite where Python's raises."""
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.copysign(INF, x)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
UC = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 512, 513)          # every cw of 1..4, and the splits 5 -> 3 + 2 and 9 -> 3 + 3 + 3
URS = (1, 7, 8, 9, 16, 17)
LARGER = ((256, 32, 32), (256, 64, 64), (16, 16, 320), (72, 72, 72), (128, 128, 128), (256, 256, 256), (512, 512, 512))          # the clamps' middles, the measured shapes
# (accepted, refused) pairs at the three limits, with the plane count and the refusal
LIMITS = (((1106,) * 3, (1107,) * 3, 2, PLAN_RUN_IDS), ((1280,) * 3, (1281,) * 3, 1, PLAN_RUN_IDS),
          ((1, 1, 524280), (1, 1, 524281), 1, PLAN_AXIS), ((1, 524280, 1), (1, 524281, 1), 1, PLAN_AXIS),
          ((1, 1, 524280), (1, 1, 524281), 2, PLAN_AXIS), ((2048, 1024, 1023), (2048, 1024, 1024), 1, PLAN_KEYS))
KEYS = (1, 2047, 2048, 2049, 2 ** 25 - 1, 2 ** 25, 2 ** 25 + 1, 2 ** 26 + 1, 2 ** 31 - 1)
KEY_TILES = (0, 1, 1000)


def plan_cases():
    boxes = [(uc, ur, us) for uc in UC for ur in URS for us in URS] + list(LARGER) + [b for lim in LIMITS for b in lim[:2]]
    boxes += [(2 ** 31 - 1, 1, 1), (1, 2 ** 31 - 1, 1), (1, 1, 2 ** 31 - 1)]          # (an axis at the end of int32: nothing wraps on the way to the refusal)
    return [(b[0], b[1], b[2], planes, worst, labels) for b in dict.fromkeys(boxes) for planes in (1, 2) for worst in (0, 1) for labels in (0, 1)]


def shift_bounds():
    out = [0.0, 5e-324]
    for k in (-1074, -1022, 0, 21, 22, 60, 61, 62, 1023):
        x = math.ldexp(1.0, k)
        out += [math.nextafter(x, 0.0), x, math.nextafter(x, INF)]
    return out + [FLT_MAX * 2.0 ** 31, 1e308, INF, NAN, -1.0]


BOX_VOX = (1, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1, 2 ** 31 - 1)
BOX_TOP = (0.0, math.ldexp(1.0, -149), 1.0, 3.5, 1e-30, FLT_MAX)
COARSE = (1, 2 ** 22, 2 ** 22 + 1, 2 ** 23, 2 ** 23 + 1, 2 ** 31 - 1)
COARSE_MUL = (math.ldexp(1.0, 40), math.ldexp(1.0, -900), math.ldexp(1.0, 900))
MAPQ = [(s, m) for s in (0.0, 1.0, 12345.678, 1e300, INF, NAN) for m in (0.0, 1e-3, 7.0, FLT_MAX, 1e305, INF, NAN)]
MODEL = ((0, 1.0), (5, 0.0), (1, 5e-324), (2 ** 22, 1.0), (1, math.nextafter(2.0 ** 22, 0.0)), (1, 2.0 ** 22), (1, math.nextafter(2.0 ** 22, INF)),
         (1000, 123.456), (1, 1e300), (2 ** 31 - 1, 1e300), (3, NAN), (1, -2.0))
TILES = ((1, 1, 1, 4, 8, 8), (0, 5, 5, 8, 8, 4), (5, 5, 0, 8, 8, 4), (17, 9, 5, 16, 8, 4), (16, 8, 4, 16, 8, 4), (1, 1, 524280, 4, 8, 8), (1, 524281, 1, 4, 8, 8),
         (2 ** 20, 2 ** 20, 2 ** 20, 1, 1, 1), (2 ** 11, 2 ** 10, 2 ** 10, 1, 1, 1), (2 ** 11, 2 ** 10, 2 ** 10 - 1, 1, 1, 1), (2 ** 31 - 1, 1, 1, 1, 8, 8),
         (2 ** 31 - 1, 1, 1, 16, 8, 4), (1, 2 ** 31 - 1, 1, 16, 8, 4))          # (an axis within a tile edge of 2^31: the round-up must not wrap)


def fmt(x):
    return x.hex() if isinstance(x, float) else str(x)


def build_cases():
    """(record, expected line) pairs."""
    out = []
    for t in TILES:
        out.append((("tiles",) + t, "tiles %d %d %d %d %d" % tile_grid(t[:3], *t[3:])))
    for c in plan_cases():
        p = plan_whole_map(*c)
        out.append((("plan",) + c, "plan " + " ".join(str(p[f]) for f in PLAN_FIELDS)))
    for keys in KEYS:
        for nt in KEY_TILES:
            k = plan_key_table(keys, nt)
            out.append((("keys", keys, nt), "keys " + " ".join(str(k[f]) for f in KEY_FIELDS)))
    for b in shift_bounds():
        out.append((("shift", b), "shift %d" % quantum_shift(b)))
    for s, m in MAPQ:
        refused, mul = map_quantum(s, m)
        out.append((("mapq", s, m), "mapq %d %s" % (refused, fmt(mul))))
    for top in BOX_TOP:
        for n in BOX_VOX:
            out.append((("boxq", top, n), "boxq %s" % fmt(box_quantum(top, n))))
    for mul in COARSE_MUL:
        for n in COARSE:
            out.append((("coarse", mul, n), "coarse %s" % fmt(mul * 0.5 ** halvings(n))))
    for n, a in MODEL:
        out.append((("model", n, a), "model %d" % model_shift(n, a)))
    return out


def canon(line):
    """A harness line with its hexadecimal floats parsed: the C library and Python spell the same double differently."""
    t = line.split()
    if t[0] in ("mapq", "boxq", "coarse"):
        t[-1] = float.fromhex(t[-1])
    return t


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("jobplan")
    exe, case_file = str(d / "jobplan_harness"), str(d / "cases.txt")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "jobplan_harness.cpp"), "-o", exe])
    cases = build_cases()
    with open(case_file, "w") as f:
        for record, _ in cases:
            f.write(" ".join(fmt(x) for x in record) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return cases, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    """No sanitizer report, and none of the invariants the harness asserts for accepted plans and key tables missed."""
    cases, proc = run
    assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-4000:]


def test_every_line_equals_the_restatement(run):
    cases, proc = run
    got = proc.stdout.splitlines()
    for g, (record, want) in zip(got, cases):
        assert canon(g) == canon(want), record
    assert len(got) == len(cases)


# ---- the restatement itself: the limits, the clamps and the bounds it must reproduce -----------------------------------------------
def test_limits_of_a_whole_map_job():
    for ok, refused, planes, code in LIMITS:
        for worst in (0, 1):
            assert plan_whole_map(*ok, planes, worst, 1)["refusal"] == PLAN_OK, ok
            assert plan_whole_map(*refused, planes, worst, 1)["refusal"] == code, refused
    assert 2048 * 1024 * 1024 == 2 ** 31
    p = plan_whole_map(1107, 1107, 1107, 2, 0, 0)
    assert p["run_ids_needed"] == p["tile_runs"] + p["worst_unit"] >= 2 ** 31 > plan_whole_map(1106, 1106, 1106, 2, 0, 0)["run_ids_needed"]
    assert plan_whole_map(1107, 1107, 1107, 1, 0, 0)["refusal"] == PLAN_OK          # (the single-sign job of the same box still fits)


def test_tile_widths_and_both_sides_of_each_clamp():
    widths = {uc: (plan_whole_map(uc, 8, 8, 1, 0, 0)["ctiles"], plan_whole_map(uc, 8, 8, 1, 0, 0)["cw"]) for uc in UC}
    assert widths[1] == widths[64] == (1, 1) and widths[65] == widths[128] == (1, 2) and widths[129] == widths[192] == (1, 3) and widths[193] == widths[256] == (1, 4)
    assert widths[257] == widths[320] == widths[321] == (2, 3) and widths[512] == (2, 4) and widths[513] == (3, 3)          # 5 -> 3 + 2, 9 -> 3 + 3 + 3
    unit, blobs = set(), set()
    for c in plan_cases():
        p = plan_whole_map(*c)
        if p["refusal"] or c[4]:
            assert p["refusal"] or (p["unit_ids"], p["max_blobs"]) == (p["worst_unit"], p["worst_blobs"])
            continue
        unit.add("worst" if p["unit_ids"] == p["worst_unit"] else "floor" if p["unit_ids"] == 65536 else "quarter")
        blobs.add("worst" if p["max_blobs"] == p["worst_blobs"] else "floor" if p["max_blobs"] == 4096 else "keys")
        assert p["unit_ids"] != 65536 or p["tile_runs"] // 4 <= 65536 <= p["worst_unit"]
        assert p["max_blobs"] != 4096 or p["total_keys"] // 32 <= 4096 <= p["worst_blobs"]
    assert unit == {"worst", "floor", "quarter"} and blobs == {"worst", "floor", "keys"}


def test_key_table_switches_groups_at_2p25_keys():
    at, over = plan_key_table(2 ** 25, 1000), plan_key_table(2 ** 25 + 1, 1000)
    assert (at["fine_shift"], at["n_groups"], at["has_group_count"]) == (4, 1024, 0)
    assert (over["fine_shift"], over["n_groups"], over["has_group_count"]) == (5, 513, 1)
    assert plan_key_table(2 ** 25 + 1, 0)["has_group_count"] == 0
    assert 2 * 256 ** 3 == 2 ** 25          # 256^3 fused is the last job of 16-counter groups
    for keys in KEYS:
        k = plan_key_table(keys, 7)
        assert k["n_groups"] <= KEY_GROUPS and k["n_fine_alloc"] >= k["n_fine"] and (k["fine_per_group"] == 16 or (KEY_GROUPS << (k["fine_shift"] - 1)) < k["n_fine"])


def test_quantum_keeps_the_bound_between_2p60_and_2p61():
    """Exact integers: whenever the shift is not clamped, bound * 2^S lies in [2^60, 2^61)."""
    seen = 0
    for b in shift_bounds():
        S = quantum_shift(b)
        if not (b > 0.0 and math.isfinite(b)):
            assert S == 40
            continue
        if -900 < S < 900:
            assert 2 ** 60 <= Fraction(b) * Fraction(2) ** S < 2 ** 61, b
            seen += 1
        else:
            assert (S == 900 and Fraction(b) * Fraction(2) ** 900 < 2 ** 61) or (S == -900 and b >= 2.0 ** 960)
    assert seen == 19 and quantum_shift(1.0) == 60 and quantum_shift(math.nextafter(1.0, 0.0)) == 61 and quantum_shift(2.0 ** 61) == -1
    assert [halvings(n) for n in COARSE] == [0, 0, 1, 1, 2, 9]
    assert all(map_quantum(s, m)[0] == (0 if math.isfinite(s) and math.isfinite(m) else 1) for s, m in MAPQ) and sum(map_quantum(s, m)[0] for s, m in MAPQ) == 22
    # a voxel's |F| < 2^39 under the map's quantum, and 2^22 of them below 2^61
    for s, m in MAPQ:
        refused, mul = map_quantum(s, m)
        if not refused and 0.0 < m <= FLT_MAX and 2.0 ** -900 < mul < 2.0 ** 900:          # (a map's voxels are floats)
            assert Fraction(m) * Fraction(mul) < 2 ** 39 and Fraction(s) * Fraction(mul) < 2 ** 61
    assert model_shift(2 ** 22, 1.0) == 40 and model_shift(1, math.nextafter(2.0 ** 22, INF)) == 39 and model_shift(1, 1e300) < 0 and model_shift(0, 1.0) == 40
