"""The host's planner of cell grids (pdb_eda_amd/csrc/pdbeda_cellgrid.h) on a CPU: tests/cellgrid_harness.cpp, built with the host compiler
under AddressSanitizer + UBSan (float-cast-overflow included, nothing recovered, nothing preloaded), against a restatement in Python floats
(fp64, unfused: the library builds with -ffp-contract=off): contacts_cases.cell_grid for make_cell_grid, and here the crop box, the corners'
bounding box (crs2xyz in the device's operation order, its fma exact through fractions) and the reach rule.  Every double is compared
through its bit pattern, every integer with ==.

What the planner promises: a grid of 1 .. 2^22 cells whose edge is above the cutoff for every box of finite, non-negative extent, and a
refusal -- not a loop without end -- for any other.  The harness is one process over one file of cases under a time limit; a sanitizer
report ends it with a non-zero status."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import batch_limit_cases
import contacts_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
STEP_LIMIT = float(1 << 29)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def grid_of(lo, hi, cutoff, n_points, crop_lo, crop_hi):
    """make_cell_grid: {lo, edge, crop_lo, crop_hi, dim, n_cells, steps}, or None where it refuses."""
    made = contacts_cases.cell_grid(lo, hi, cutoff, n_points)
    if made is None:
        return None
    edge, dims, n_cells, steps = made
    return dict(lo=[float(v) for v in lo], edge=edge, crop_lo=[float(v) for v in crop_lo], crop_hi=[float(v) for v in crop_hi], dim=dims, n_cells=n_cells, steps=steps)


def bad_axis(lo, hi):
    for q in range(3):
        e = float(hi[q]) - float(lo[q])
        if not (e >= 0.0 and math.isfinite(e)):
            return q
    return -1


def query_box(q, cutoff):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        return [float(v) - 2 * float(cutoff) for v in q.min(axis=0)], [float(v) + 2 * float(cutoff) for v in q.max(axis=0)]


def crop_grid(blo, bhi, reach, xyz):
    """crop_cell_grid: the box grown by the reach, its intersection with the atoms' box, one cell and no atom in it where that is empty."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    alo, ahi = ([float(v) for v in xyz.min(axis=0)], [float(v) for v in xyz.max(axis=0)]) if n else ([INF] * 3, [-INF] * 3)
    reach = float(reach)
    crop_lo, crop_hi, glo, ghi, empty = [], [], [], [], n == 0
    for q in range(3):
        pad = reach * (1.0 + 1e-5) + 1e-8 * ((abs(float(blo[q])) + abs(float(bhi[q]))) + 1.0)
        crop_lo.append(float(blo[q]) - pad)
        crop_hi.append(float(bhi[q]) + pad)
        glo.append(max(crop_lo[q], alo[q]))
        ghi.append(min(crop_hi[q], ahi[q]))
        if not glo[q] <= ghi[q]:
            empty = True
    if empty:
        glo, ghi = list(crop_lo), list(crop_lo)
    return grid_of(glo, ghi, reach, n, crop_lo, crop_hi), empty


def held_cells(g, xyz):
    """grid_cropped / grid_cell of every atom: its cell number, -1 where it is cropped."""
    out = []
    for v in np.asarray(xyz, dtype=np.float64).reshape(-1, 3):
        if not all(g["crop_lo"][q] <= float(v[q]) <= g["crop_hi"][q] for q in range(3)):
            out.append(-1)
            continue
        c = [min(max(math.floor((float(v[q]) - g["lo"][q]) / g["edge"]), 0), g["dim"][q] - 1) for q in range(3)]
        out.append((c[2] * g["dim"][1] + c[1]) * g["dim"][0] + c[0])
    return out


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # (int / int is correctly rounded: one rounding, as fma)


def crs2xyz(h, crs):
    """DensityHeader.crs2xyzCoord for integer crs in the device's operation order."""
    if h.orthogonal:
        return [float(crs[h.map2xyz[i]]) * float(h.gridLength[i]) + float(h.origin[i]) for i in range(3)]
    o = np.asarray(h.orthoMat, dtype=np.float64).reshape(9)
    f = [float(crs[h.map2xyz[i]] + h.crsStart[h.map2xyz[i]]) / float(h.xyzInterval[i]) for i in range(3)]
    return [_fma(o[3 * i + 2], f[2], _fma(o[3 * i], f[0], float(o[3 * i + 1]) * f[1])) for i in range(3)]


def corners_box(h, c0, c1):
    pts = [crs2xyz(h, [(c1 if k & 1 else c0)[0], (c1 if k & 2 else c0)[1], (c1 if k & 4 else c0)[2]]) for k in range(8)]
    return [min(p[q] for p in pts) for q in range(3)], [max(p[q] for p in pts) for q in range(3)]


def per_unit(h):
    if h.orthogonal:
        return [1.0 / abs(float(h.gridLength[i])) for i in range(3)]
    d = np.asarray(h.deOrthoMat, dtype=np.float64).reshape(9)
    return [((abs(float(d[3 * i])) + abs(float(d[3 * i + 1]))) + abs(float(d[3 * i + 2]))) * float(h.xyzInterval[i]) for i in range(3)]


def reach_fits(h, reach):
    return all(float(reach) * u < STEP_LIMIT for u in per_unit(h))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _headers():
    from pdb_eda_amd import ccp4, synthetic
    return {name: ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(batch_limit_cases.spec_and_grid(name)[0])) for name in batch_limit_cases.WORLDS}


def _num(v):
    return float(v).hex()


def _geom_line(h):
    nums = list(h.origin) + list(h.gridLength) + list(np.asarray(h.orthoMat, dtype=np.float64).reshape(9)) + list(np.asarray(h.deOrthoMat, dtype=np.float64).reshape(9))
    ints = [int(bool(h.orthogonal))] + list(h.map2xyz) + list(h.crsStart) + list(h.xyzInterval)
    return "geom " + " ".join(str(int(v)) for v in ints) + " " + " ".join(_num(v) for v in nums)


def _grid_line(g):
    vals = g["lo"] + [g["edge"]] + g["crop_lo"] + g["crop_hi"]
    return "grid " + " ".join(bits(v) for v in vals) + " %d %d %d %d" % (*g["dim"], g["n_cells"])


class Cases(object):
    def __init__(self):
        self.lines, self.want, self.where = [], [], []      # the file, the expected output, which case an output line belongs to

    def add(self, name, record, want):
        self.lines += record
        self.want += want
        self.where += [name] * len(want)

    def grid(self, name, lo, hi, cutoff, n_points):
        g = grid_of(lo, hi, cutoff, n_points, lo, hi)
        self.add(name, ["grid %s %s %s %d" % (" ".join(_num(v) for v in lo), " ".join(_num(v) for v in hi), _num(cutoff), n_points)],
                 [_grid_line(g) if g else "refused %d" % bad_axis(lo, hi)])
        return g

    def query(self, name, q, cutoff, n_points):
        lo, hi = query_box(q, cutoff)
        g = grid_of(lo, hi, cutoff, n_points, lo, hi)
        self.add(name, ["query %d %s %d" % (len(q), _num(cutoff), n_points)] + [" ".join(_num(v) for v in p) for p in q], [_grid_line(g) if g else "refused %d" % bad_axis(lo, hi)])
        return g

    def crop(self, name, blo, bhi, reach, xyz):
        g, empty = crop_grid(blo, bhi, reach, xyz)
        held = held_cells(g, xyz)
        self.add(name, ["crop %s %s %s %d" % (" ".join(_num(v) for v in blo), " ".join(_num(v) for v in bhi), _num(reach), len(xyz))] + [" ".join(_num(v) for v in p) for p in xyz],
                 [_grid_line(g), " ".join(["held"] + [str(c) for c in held])])
        return g, empty, held

    def corners(self, name, h, c0, c1):
        lo, hi = corners_box(h, c0, c1)
        self.add(name, ["corners %d %d %d %d %d %d" % (*c0, *c1)], ["corners " + " ".join(bits(v) for v in lo + hi)])
        return lo, hi

    def reach(self, name, h, r):
        fits = reach_fits(h, r)
        self.add(name, ["reach " + _num(r)], ["reach %d" % fits])
        return fits


def _build_cases():
    cs = Cases()
    rng = np.random.default_rng(2203)
    # ---- make_cell_grid ----
    g = cs.grid("a single point", [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 5.0, 1)
    assert g["dim"] == (1, 1, 1) and g["steps"] == 0
    g = cs.grid("no point", [0.0, 0.0, 0.0], [3.0, 3.0, 3.0], 1.0, 0)
    assert g["n_cells"] == 27 and g["steps"] == 0
    # 20^3 = 8 000 cells at the first edge: above the floor of 4 096 for few points, inside 8 per point from 1 000 points on
    for n_points, steps in ((0, 1), (10, 1), (512, 1), (999, 1), (1000, 0), (5000, 0)):
        g = cs.grid("the floor and 8 cells a point, %d points" % n_points, [0.0] * 3, [19.5] * 3, 1.0, n_points)
        assert (g["steps"] > 0) == bool(steps) and g["n_cells"] <= max(4096, 8 * n_points), (n_points, g)
    assert cs.grid("exactly 4096 cells", [0.0] * 3, [15.5] * 3, 1.0, 3)["n_cells"] == 4096
    g = cs.grid("coarsened to the cap", [-500.0, -400.0, -300.0], [500.0, 600.0, 700.0], 1.0, 10 ** 7)
    assert g["steps"] >= 1 and (1 << 22) // 8 < g["n_cells"] <= 1 << 22 and g["edge"] > 1.0
    g = cs.grid("flat and long", [0.0, 7.0, -3.0], [1e7, 7.0, -3.0], 0.25, 100)
    assert g["steps"] >= 1 and g["dim"][1:] == (1, 1)
    g = cs.grid("extents of 1e300", [-5e299, 0.0, -1e300], [5e299, 1e300, 0.0], 1.0, 1000)
    assert g["steps"] > 3000 and 1 <= g["n_cells"] <= 8000 and math.isfinite(g["edge"])
    for axis in range(3):
        lo, hi = [0.0, 0.0, 0.0], [10.0, 10.0, 10.0]
        lo[axis], hi[axis] = -1e308, 1e308
        assert cs.grid("an extent that overflows along %d" % axis, lo, hi, 1.0, 100) is None and bad_axis(lo, hi) == axis
    assert cs.grid("an extent that overflows by 1 ulp", [-float(np.finfo(np.float64).max) / 2] * 3, [float(np.nextafter(np.finfo(np.float64).max / 2, INF))] * 3, 1.0, 9) is None
    assert cs.grid("the largest finite extent", [-float(np.finfo(np.float64).max) / 2] * 3, [float(np.finfo(np.float64).max) / 2] * 3, 1.0, 9) is not None
    assert cs.grid("a negative extent", [0.0, 5.0, 0.0], [1.0, 4.0, 1.0], 1.0, 9) is None
    assert cs.grid("the box of no point", [INF] * 3, [-INF] * 3, 1.0, 0) is None
    # ---- query_grid ----
    q = np.round(rng.uniform(-20.0, 20.0, (50, 3)), 3)
    g = cs.query("ordinary queries", q, 1.7, 5050)
    assert g["crop_lo"] == g["lo"] and g["lo"][0] == float(q[:, 0].min()) - 3.4
    assert cs.query("one query", q[:1], 2.5, 2)["dim"] == (4, 4, 4)      # (4 cutoffs wide, edge just above one)
    far = np.concatenate([[[1e308, 0.0, 0.0], [-1e308, 0.0, 0.0]], q[:5]])
    assert cs.query("two queries at +-1e308", far, 1.7, 107) is None
    assert cs.query("queries whose grown box overflows", [[-1.7e308, 0.0, 0.0], [0.0, 1.0, 2.0]], 1e308, 2) is None
    # ---- crop_cell_grid ----
    box = ([0.0, -4.0, 2.0], [23.5, 15.5, 19.5])
    atoms = np.round(rng.uniform(-12.0, 32.0, (300, 3)), 3)
    g, empty, held = cs.crop("atoms all round the box", *box, 3.5, atoms)
    assert not empty and 0 < held.count(-1) < 300 and len(set(held)) > 20
    g, empty, held = cs.crop("atoms inside the box", *box, 3.5, np.round(rng.uniform(3.0, 12.0, (40, 3)), 3))
    assert not empty and -1 not in held and g["lo"][0] >= 3.0 and g["crop_lo"][0] < -3.5
    g, empty, held = cs.crop("no atom", *box, 3.5, np.zeros((0, 3)))
    assert empty and g["n_cells"] == 1 and g["lo"] == g["crop_lo"]
    for axis in range(3):
        beside = np.round(rng.uniform(3.0, 12.0, (25, 3)), 3)
        beside[:, axis] += 60.0
        g, empty, held = cs.crop("atoms beside the box along %d" % axis, *box, 3.5, beside)
        assert empty and g["n_cells"] == 1 and g["lo"] == g["crop_lo"] and held == [-1] * 25
    g, empty, held = cs.crop("one atom on the crop box's face", *box, 3.5, [[crop_grid(*box, 3.5, [])[0]["crop_hi"][0], 1.0, 5.0]])
    assert not empty and held == [0] and g["n_cells"] == 1
    g, empty, held = cs.crop("a reach that carries its own factor", [-7.25, 0.5, 3.0], [11.0, 9.75, 3.0], 2.0 * 4.5 * (1.0 + 1e-6), np.round(rng.uniform(-20.0, 25.0, (120, 3)), 3))
    assert not empty and 0 < held.count(-1) < 120
    g, empty, held = cs.crop("a huge crowd far round a small box", [0.0] * 3, [4.0] * 3, 1.5, np.round(rng.uniform(-400.0, 400.0, (2000, 3)), 2))
    assert g["dim"][0] <= 6 and held.count(-1) > 1990      # (the grid does not grow with atoms far from the box)
    # ---- the worlds: corners and the reach rule ----
    for world, h in _headers().items():
        cs.lines.append(_geom_line(h))
        n = list(h.ncrs)
        lo, hi = cs.corners(world + " the stored box", h, [0, 0, 0], [n[0] - 1, n[1] - 1, n[2] - 1])
        assert all(lo[q] < hi[q] for q in range(3))
        if not h.orthogonal:      # skewed: no single corner holds the box's low end on every axis
            pts = [crs2xyz(h, [(n[0] - 1) * (k & 1), (n[1] - 1) * ((k >> 1) & 1), (n[2] - 1) * (k >> 2)]) for k in range(8)]
            assert lo not in pts and hi not in pts
        cs.corners(world + " one voxel", h, [5, 6, 7], [5, 6, 7])
        cs.corners(world + " a clamped tile", h, [32, 36, 32], [47, 39, 35])
        cs.corners(world + " outside the box", h, [-9, -3, 40], [-2, 60, 41])
        g, empty, held = cs.crop(world + " atoms round the map", lo, hi, 3.5, np.round(rng.uniform(np.array(lo) - 8.0, np.array(hi) + 8.0, (200, 3)), 3))
        assert not empty and 0 < held.count(-1) < 200
        # exactly at 2^29 steps (refused), just below (accepted): along the axis that takes the most steps a unit
        unit = max(per_unit(h))
        r = STEP_LIMIT / unit
        while reach_fits(h, r):
            r = float(np.nextafter(r, INF))
        below = float(np.nextafter(r, 0.0))
        assert r * unit >= STEP_LIMIT > below * unit
        if h.orthogonal:
            assert r * unit == STEP_LIMIT      # (0.5 A voxels: 2^28 A are 2^29 steps to the bit)
        assert not cs.reach(world + " a reach of 2^29 steps", h, r) and cs.reach(world + " the reach just below", h, below)
        assert cs.reach(world + " an ordinary reach", h, 3.5) and not cs.reach(world + " an infinite reach", h, INF) and not cs.reach(world + " a NaN reach", h, float("nan"))
    return cs


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("cellgrid")
    exe, case_file = str(d / "cellgrid_harness"), str(d / "cases.txt")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cellgrid_harness.cpp"), "-o", exe])
    cs = _build_cases()
    with open(case_file, "w") as f:
        f.write("\n".join(cs.lines) + "\n")
    proc = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=120)      # (a planner that never returns fails here)
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


def test_overflowing_extents_are_refused(run):
    cs, proc = run
    got = proc.stdout.splitlines()
    refused = [i for i, name in enumerate(cs.where) if "overflow" in name or "+-1e308" in name]
    assert len(refused) >= 6 and all(got[i].startswith("refused ") and got[i] == cs.want[i] for i in refused)
