"""The host's planner of sphere batches (pdb_eda_amd/csrc/pdbeda_spherebox.h) on a CPU: tests/spherebox_harness.cpp, built with the host
compiler under AddressSanitizer + UBSan (float-cast-overflow included, nothing recovered, nothing preloaded), against a restatement of
xyzCoord -> crs (np.rint, the header's axis permutation; the matrix product in the device's fma order, exact through fractions) and of
the box / volume rule in numpy and Python integers.  Everything is compared with ==.

What the planner promises: it casts nothing it has not tested (a coordinate is plannable when it is finite and every grid index is below
2^29 in magnitude, a radius when it is finite, >= 0 and its half-widths are), and it lays out only what fits ONE limit (every width
below 2^30, the batch below 2^31 mask words and 2^40 keys; a volume has at most 64 keys a word, so the words decide).  The harness is
one process over one file of cases; a sanitizer report ends it with a non-zero status."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import batch_limit_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_LIMIT, WIDTH_LIMIT, WORDS_LIMIT, KEYS_LIMIT, SMALL_ROWS = 1 << 29, 1 << 30, 1 << 31, 1 << 40, 512
RADII = [0.0, 0.7, 1.9, 3.5]
EMPTY = ([0, 0, 0], [-1, -1, -1])


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # (int / int is correctly rounded: one rounding, as fma)


def crs_of(h, xyz):
    """DensityHeader.xyz2crsCoord in the device's operation order; None: not plannable."""
    xyz = [float(v) for v in xyz]
    if not all(np.isfinite(xyz)):
        return None
    if h.orthogonal:
        with np.errstate(over="ignore"):
            pos = [float((np.float64(xyz[i]) - np.float64(h.origin[i])) / np.float64(h.gridLength[i])) for i in range(3)]
        start = [0, 0, 0]
    else:
        a = np.asarray(h.deOrthoMat, dtype=np.float64).reshape(9)
        f = [_fma(a[3 * i + 2], xyz[2], _fma(a[3 * i], xyz[0], float(a[3 * i + 1]) * xyz[1])) for i in range(3)]
        pos = [f[i] * float(h.xyzInterval[i]) for i in range(3)]
        start = [h.crsStart[h.map2xyz[i]] for i in range(3)]
    if not all(np.isfinite(pos)):
        return None
    grid = [int(np.rint(pos[i])) - start[i] for i in range(3)]
    crs = [grid[h.map2crs[i]] for i in range(3)]
    return crs if all(abs(c) < INDEX_LIMIT for c in crs) else None


def half_widths(h, rad):
    rad = float(np.float32(rad))
    if not np.isfinite(rad) or not rad >= 0.0:
        return None
    return crs_of(h, [float(h.origin[i]) + rad for i in range(3)])


def box_of(C, R):
    lo, hi = np.asarray(C, dtype=np.int64) - np.asarray(R, dtype=np.int64) - 1, np.asarray(C, dtype=np.int64) + np.asarray(R, dtype=np.int64)
    return EMPTY if np.any(hi < lo) else (lo.tolist(), hi.tolist())


def finish(bounds):
    """[(lo, hi)] per group -> (fits, vol lines, words, keys, small_boxes, largest)."""
    words = keys = largest = 0
    fits, small, vols = True, True, []
    for g, (lo, hi) in enumerate(bounds):
        dim = [0, 0, 0] if any(hi[k] < lo[k] for k in range(3)) else [int(hi[k]) - int(lo[k]) + 1 for k in range(3)]
        org = [0, 0, 0] if dim == [0, 0, 0] else [int(v) for v in lo]
        row_words = (dim[0] + 63) // 64
        vols.append("vol %d %d %d %d %d %d %d %d %d %d" % (*dim, *org, row_words, g, words, keys))
        fits = fits and all(d < WIDTH_LIMIT for d in dim)
        small = small and row_words <= 1 and dim[1] * dim[2] <= SMALL_ROWS
        largest = max(largest, dim[0] * dim[1] * dim[2])
        words += row_words * dim[1] * dim[2]
        keys += dim[0] * dim[1] * dim[2]
    fits = fits and words < WORDS_LIMIT and keys < KEYS_LIMIT
    return fits, vols, words, keys, small, largest


def plan_line(plannable, fits, words=0, keys=0, small=False, largest=0):
    head = "plan plannable %d fits %d" % (plannable, fits)
    return head + (" small_boxes %d words %d keys %d largest %d" % (small, words, keys, largest) if fits else "")


def group_bounds(boxes, groups, n_groups):
    lo, hi = [[None] * 3 for _ in range(n_groups)], [[None] * 3 for _ in range(n_groups)]
    for (blo, bhi), g in zip(boxes, groups):
        if bhi[0] < blo[0]:
            continue
        for k in range(3):
            lo[g][k] = blo[k] if lo[g][k] is None else min(lo[g][k], blo[k])
            hi[g][k] = bhi[k] if hi[g][k] is None else max(hi[g][k], bhi[k])
    return [EMPTY if lo[g][0] is None else (lo[g], hi[g]) for g in range(n_groups)]


def expect_spheres(h, atoms, n_groups, grouped):
    """The lines the harness prints for one `spheres` record."""
    boxes, plannable = [], True
    for xyz, rad, _ in atoms:
        R, C = half_widths(h, rad), crs_of(h, xyz)
        if R is None or C is None:
            plannable = False
            break
        boxes.append(box_of(C, R))
    out = [plan_line(0, 0)]
    if plannable:
        fits, vols, words, keys, small, largest = finish(group_bounds(boxes, [g for _, _, g in atoms], n_groups) if grouped else boxes)
        out = [plan_line(1, fits, words, keys, small, largest)]
        if fits:
            out += ["box %d %d %d %d %d %d" % (*lo, *hi) for lo, hi in boxes] + vols
    if not grouped:      # the totals from the radii alone: the box of an atom at index 0 stands for its radius
        widths = [half_widths(h, rad) for _, rad, _ in atoms]
        if any(R is None for R in widths):
            out.append("radii " + plan_line(0, 0))
        else:
            fits, _, words, keys, small, largest = finish([box_of([0, 0, 0], R) for R in widths])
            out.append("radii " + plan_line(1, fits, words, keys, small, largest))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _headers():
    from pdb_eda_amd import ccp4, synthetic
    specs = {name: batch_limit_cases.spec_and_grid(name)[0] for name in batch_limit_cases.WORLDS}
    ncrs = synthetic.BIG_CASES["c5_hex_perm"][0]
    specs["hex_perm"] = synthetic.MapSpec(ncrs=tuple(ncrs), spacing=synthetic.BIG_CASES["c5_hex_perm"][3], **synthetic.BIG_CASE_SPECS["c5_hex_perm"])
    return {name: ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(spec)) for name, spec in specs.items()}


def _geom_line(h):
    nums = [float(v).hex() for v in list(h.origin) + list(h.gridLength) + list(np.asarray(h.deOrthoMat, dtype=np.float64).reshape(9))]
    ints = [int(bool(h.orthogonal))] + list(h.map2xyz) + list(h.map2crs) + list(h.crsStart) + list(h.xyzInterval)
    return "geom " + " ".join(str(int(v)) for v in ints) + " " + " ".join(nums)


def _num(v):
    return float(v).hex()


def _last_radius_inside(h):
    """The largest float32 radius whose half-widths plan (bisection over the float32 bit patterns, by the restatement)."""
    bits = lambda r: int(np.float32(r).view(np.int32))
    lo, hi = bits(1.0), bits(3.0e38)
    assert half_widths(h, np.int32(lo).view(np.float32)) is not None and half_widths(h, np.int32(hi).view(np.float32)) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if half_widths(h, np.int32(mid).view(np.float32)) is not None:
            lo = mid
        else:
            hi = mid
    return float(np.int32(lo).view(np.float32)), float(np.int32(hi).view(np.float32))


class Cases(object):
    def __init__(self):
        self.lines, self.want, self.where = [], [], []      # the file, the expected output, which case an output line belongs to

    def add(self, name, record, want):
        self.lines += record
        self.want += want
        self.where += [name] * len(want)

    def crs(self, name, h, xyz):
        c = crs_of(h, xyz)
        self.add(name, ["crs " + " ".join(_num(v) for v in xyz)], ["crs %d %d %d %d" % ((1, *c) if c else (0, 0, 0, 0))])
        return c

    def half(self, name, h, rad):
        R = half_widths(h, rad)
        self.add(name, ["halfwidths " + _num(np.float32(rad))], ["halfwidths %d %d %d %d" % ((1, *R) if R else (0, 0, 0, 0))])
        return R

    def spheres(self, name, h, atoms, n_groups, grouped):
        want = expect_spheres(h, atoms, n_groups, grouped)
        rec = ["spheres %d %d %d" % (len(atoms), n_groups, grouped)] + ["%s %s %s %s %d" % (*[_num(v) for v in xyz], _num(np.float32(rad)), g) for xyz, rad, g in atoms]
        self.add(name, rec, want)
        return want

    def bounds(self, name, n_groups, boxes):
        """boxes: (group_a, group_b, lo, hi); the box joins both groups (-1: none)."""
        joined = [(lo, hi) for ga, gb, lo, hi in boxes for g in (ga, gb) if g >= 0]
        fits, vols, words, keys, small, largest = finish(group_bounds(joined, [g for ga, gb, _, _ in boxes for g in (ga, gb) if g >= 0], n_groups))
        want = [plan_line(1, fits, words, keys, small, largest)] + (vols if fits else [])
        self.add(name, ["bounds %d %d" % (n_groups, len(boxes))] + ["%d %d %d %d %d %d %d %d" % (ga, gb, *lo, *hi) for ga, gb, lo, hi in boxes], want)
        return fits, words, keys


def _build_cases():
    cs = Cases()
    rng = np.random.default_rng(1629)
    for world, h in _headers().items():
        cs.lines.append(_geom_line(h))
        nc = np.array(h.ncrs)
        inside = [np.asarray(h.crs2xyzCoord([int(v) for v in rng.integers(-4, nc + 4)]), dtype=np.float64) + rng.uniform(-0.3, 0.3, 3) for _ in range(7)]
        for p in inside:
            assert cs.crs(world + " inside", h, p) is not None
        # half-way between grid points along each axis, both parities (exact ties on the orthogonal world, whose origin is 0 and spacing 0.5)
        for axis in range(3):
            for k in (6, 7, -6, -7):
                idx = np.array([10.0, 11.0, 12.0])
                idx[axis] = k + 0.5
                p = [idx[h.map2xyz[i]] * h.gridLength[i] + h.origin[i] for i in range(3)] if h.orthogonal else h.crs2xyz_array(idx[None, :])[0]
                c = cs.crs(world + " tie", h, p)
                if h.orthogonal:
                    assert c[axis] == int(np.rint(k + 0.5)) and c[axis] % 2 == 0, (world, axis, k, c)
        # +-(2^29 - 1) and +-2^29 grid steps along each axis
        for axis in range(3):
            for sign in (1, -1):
                for steps, plans in ((INDEX_LIMIT - 1, True), (INDEX_LIMIT, False), (INDEX_LIMIT - 3, True), (INDEX_LIMIT + 3, False)):
                    idx = np.zeros(3)
                    idx[axis] = sign * steps
                    if h.orthogonal:
                        p = [idx[h.map2xyz[i]] * h.gridLength[i] + h.origin[i] for i in range(3)]
                    else:      # (crs2xyz lands within a rounding error of the index: the restatement says on which side, three steps off leave no doubt)
                        p = h.crs2xyz_array(idx[None, :])[0]
                    c = cs.crs(world + " edge", h, p)
                    if h.orthogonal or steps in (INDEX_LIMIT - 3, INDEX_LIMIT + 3):
                        assert (c is not None) == plans, (world, axis, sign, steps, c)
                    if c is not None:
                        assert abs(c[axis]) < INDEX_LIMIT
        # what no cast may see
        for axis in range(3):
            for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300):
                p = np.array(inside[0])
                p[axis] = bad
                assert cs.crs(world + " unplannable", h, p) is None
                want = cs.spheres(world + " unplannable batch", h, [(inside[1], 0.7, 0), (p, 0.7, 1), (inside[2], 0.7, 2)], 3, 0)
                assert want[0] == plan_line(0, 0) and want[-1].startswith("radii plan plannable 1 fits 1")
        for bad in (np.nan, np.inf, -np.inf, -0.5, 1e30):
            assert cs.half(world + " bad radius", h, bad) is None
            want = cs.spheres(world + " bad radius batch", h, [(inside[1], 0.7, 0), (inside[2], bad, 1)], 2, 0)
            assert want == [plan_line(0, 0), "radii " + plan_line(0, 0)]
        for rad in RADII:
            assert cs.half(world + " radius", h, rad) is not None
        last_in, first_out = _last_radius_inside(h)
        R = cs.half(world + " radius edge", h, last_in)
        assert R is not None and max(abs(v) for v in R) < INDEX_LIMIT and cs.half(world + " radius edge", h, first_out) is None
        want = cs.spheres(world + " widest radius", h, [(inside[0], last_in, 0)], 1, 0)      # plannable; far beyond the one limit
        assert want[0] == plan_line(1, 0)
        # per-atom batches: n = 0, n = 1, every radius
        for n in (0, 1, 5):
            atoms = [(inside[a], RADII[(a + 1) % 4], a) for a in range(n)]
            want = cs.spheres(world + " per atom n=%d" % n, h, atoms, n, 0)
            assert want[0].startswith("plan plannable 1 fits 1") and want[-1] == "radii " + want[0], want      # (the radii-only totals ARE the plan's)
        # grouped: groups of 1 and of several atoms, an empty group; n = 0 and n = 1
        atoms = [(inside[a], RADII[a % 4], g) for a, g in enumerate([0, 1, 1, 1, 3, 3, 4])]
        want = cs.spheres(world + " grouped", h, atoms, 5, 1)
        assert want[0].startswith("plan plannable 1 fits 1") and want[1 + 7 + 2].startswith("vol 0 0 0 0 0 0 0 2 ")
        cs.spheres(world + " grouped n=0", h, [], 2, 1)
        cs.spheres(world + " grouped n=1", h, [(inside[3], 1.9, 0)], 1, 1)
    # ---- bounds: what the accumulator and the finish make of boxes, whatever made them ----
    one = ([5, 6, 7], [9, 12, 8])
    cs.bounds("all boxes of a group empty", 3, [(0, -1, *EMPTY), (1, -1, *one), (0, -1, *EMPTY)])
    # the union form: each box joins its residue group and the domain group (the last); residue group 1 stays empty
    fits, words, keys = cs.bounds("union", 4, [(0, 3, [1, 2, 3], [8, 9, 10]), (2, 3, [-5, 0, 4], [2, 3, 30]), (0, 3, [7, 7, 7], [70, 8, 9]), (2, 3, *EMPTY)])
    assert fits and words > 0
    wide = lambda w: ([-(1 << 29), 0, 0], [-(1 << 29) + w - 1, 0, 0])
    assert cs.bounds("union, one width 2^30 - 1", 3, [(0, 2, *wide((1 << 30) - 1))])[0]
    assert not cs.bounds("union, one width 2^30", 3, [(0, 2, *wide(1 << 30))])[0]
    assert not cs.bounds("union, a width 2^30 from two boxes", 2, [(0, 1, [-(1 << 29), 0, 0], [0, 0, 0]), (0, 1, [0, 0, 0], [(1 << 29) - 1, 0, 0])])[0]
    assert not cs.bounds("three widths 2^30 - 1", 1, [(0, -1, [0, 0, 0], [(1 << 30) - 2] * 3)])[0]      # (no product may leave int64 on the way to saying so)
    # totals by formula: 2^30 + (2^30 - 2^20) + rows mask words, rows = 2^20 - 1 (just below the limit) and 2^20 (at it)
    big = lambda rows_s: [(0, -1, [0, 0, 0], [65535, 1023, 1023]), (1, -1, [0, 0, 0], [65535, 1023, 1022]), (2, -1, [0, 0, 0], [63, 1023, rows_s - 1])]
    fits, words, keys = cs.bounds("totals below the limit", 3, [(0, -1, [0, 0, 0], [65535, 1023, 1023]), (1, -1, [0, 0, 0], [65535, 1023, 1022]), (2, -1, [0, 0, 0], [0, 1024, 1022])])
    assert fits and words == WORDS_LIMIT - 1 and keys < KEYS_LIMIT
    fits, words, keys = cs.bounds("totals at the limit", 3, big(1024))
    assert not fits and words == WORDS_LIMIT
    return cs


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("spherebox")
    exe, case_file = str(d / "spherebox_harness"), str(d / "cases.txt")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "spherebox_harness.cpp"), "-o", exe])
    cs = _build_cases()
    with open(case_file, "w") as f:
        f.write("\n".join(cs.lines) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)
    return cs, proc


def test_the_harness_ends_clean_under_the_sanitizers(run):
    cs, proc = run
    assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-4000:]


def test_planner_equals_the_restatement(run):
    cs, proc = run
    got = proc.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, cs.want)):
        assert g == w, (cs.where[i], i)
    assert len(got) == len(cs.want)
