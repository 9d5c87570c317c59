"""The per-atom sphere entry points (pdbeda_region_sums, pdbeda_sphere_blobs, pdbeda_radial_profiles) on both sides of the
batch sizes at which they change kernels or start to walk a batch in several trips: the staged row of group_setup (1 MiB),
the 65536-block grids of k_region_reduce and k_atom_shells, the 1024-group trips of k_make_vols and the chunks of
pdbeda_radial_profiles.

Yardsticks: tests/spheres_checker.py (region sums; pinned against the oracle by tests/test_spheres_host.py),
tests/profiles_checker.py (radial profiles) and the oracle's find_aberrant_blobs (blobs), computed on the P = 3001 distinct
positions of tests/batch_limit_cases.py and expanded by index: atom i sits on position i % P, and EVERY row of a batch is compared.
Counts, flags, voxel sets and group ids are compared with np.array_equal; a sum within 1e-9 * count * max |rho| (the bound of
tests/test_gpu_profiles.py), count being the voxels in that sum; a sum over no voxel is exactly 0.

Every case makes its call on the session's context, repeats it between profile_begin() and profile_end() on a second context,
requires the same bytes from both, and asserts on the kernel names and call counts the profile returned: the batch sizes below are
the ones at which those kernels were seen to run."""
import io
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
import batch_limit_cases as cases
import profiles_checker
import spheres_checker
from test_gpu_profiles import assert_profiles_equal

pytestmark = pytest.mark.gpu

RADIUS = 0.7          # a 4 x 4 x 4 box at 0.5 A
P = cases.P


@pytest.fixture(scope="module")
def prof_ctx():
    from pdb_eda_amd import _native
    return _native.Context(0)


@pytest.fixture(scope="module", params=cases.WORLDS)
def world(request, gpu_ctx, prof_ctx):
    from pdb_eda_amd import ccp4, synthetic
    from oracle import oracle as ora
    name = request.param
    spec, grid = cases.spec_and_grid(name)
    raw = synthetic.ccp4_bytes(spec, grid)
    w = types.SimpleNamespace(name=name, grid=grid, top=float(np.abs(grid).max()))
    w.dm = ccp4.parse(io.BytesIO(raw), name, ctx=gpu_ctx)
    w.dm_prof = ccp4.parse(io.BytesIO(raw), name, ctx=prof_ctx)
    w.prof_ctx = prof_ctx
    w.header = w.dm.header
    w.base = cases.base_atoms(name, w.header)
    w.sigma = float(w.dm.meanDensity + 1.5 * w.dm.stdDensity)
    w.oracle = ora.Oracle(w.header, grid)
    w.spheres = spheres_checker.atom_spheres(w.header, grid, w.base, RADIUS, crs2xyz=w.dm._map.crs2xyz)
    w.region = {}          # cutoff -> the checker's per-atom region sums of the P positions
    w.cache = {}
    return w


def region_want(w, cut):
    if cut not in w.region:
        want = spheres_checker.region_sums(w.header, w.grid, w.base, RADIUS, cut, spheres=w.spheres)
        assert want["cnt"].sum() > 0
        if cut != 0.0:
            assert 0 < want["n_pos"].sum() + want["n_neg"].sum() < want["cnt"].sum()
        assert want["valid"].any() and (w.name == "orth" or not want["valid"].all())          # skew: both answers
        w.region[cut] = want
    return w.region[cut]


def twice(w, call, same):
    """call(map) on the session's context, then again under the profiler on the second context: (result, {kernel: calls})."""
    first = call(w.dm._map)
    w.prof_ctx.profile_begin()
    try:
        second = call(w.dm_prof._map)
    finally:
        prof = {k: v[0] for k, v in w.prof_ctx.profile_end().items()}
    print("%s: kernels %s" % (w.name, json.dumps(prof, sort_keys=True)))
    same(first, second)
    return first, prof


def same_arrays(a, b):
    a, b = (x if isinstance(x, dict) else dict(enumerate(x)) for x in (a, b))
    assert list(a) == list(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def assert_region_equal(got, want, idx, top, what):
    """got: DeviceMap.region_sums();  want: spheres_checker.region_sums(), row idx[g] for group g."""
    pos, neg, cnt, valid = got
    assert np.array_equal(cnt, want["cnt"][idx]), what
    assert np.array_equal(valid, want["valid"][idx]), what
    for tag, mine, theirs, count in (("pos", pos, want["pos"][idx], want["n_pos"][idx]), ("neg", neg, want["neg"][idx], want["n_neg"][idx])):
        err = np.abs(mine - theirs)
        bound = 1e-9 * count * top
        print("%s: max |%s - checker| = %.3g (bound at that group %.3g), %d voxels in %d groups" %
              (what, tag, float(err.max()), float(bound[int(err.argmax())]), int(count.sum()), count.size))
        assert np.all(err <= bound), what
        assert np.all(mine[count == 0] == 0.0), what          # an empty region is exactly 0


def per_atom_region(w, n, cut):
    xyz = w.base[cases.tiled(n)]
    rad, off = np.full(n, RADIUS, dtype=np.float32), np.arange(n + 1, dtype=np.int64)
    return twice(w, lambda m: m.region_sums(xyz, rad, off, cut), same_arrays)


# ---- 1, 2: region sums, a group per atom -------------------------------------------------------------------------------------
def test_region_sums_below_and_above_the_staged_row(world):
    """8 000 atoms (a staged row of 832 kB <= 1 MiB): k_atom_region x 1, nothing else.  12 000 atoms (1.25 MB): k_init_bounds,
    k_atom_boxes, k_make_vols (12 trips of 1024 groups), k_sphere_paint and k_region_reduce, x 1 each, no k_atom_region."""
    w = world
    for cut in (w.sigma, 0.1):
        want = region_want(w, cut)
        small, prof = per_atom_region(w, 8000, cut)
        assert prof.get("k_atom_region") == 1 and "k_region_reduce" not in prof and "k_sphere_paint" not in prof, prof
        assert_region_equal(small, want, cases.tiled(8000), w.top, "%s 8000 cut=%.3g" % (w.name, cut))
        large, prof = per_atom_region(w, 12000, cut)
        assert prof.get("k_sphere_paint") == 1 and prof.get("k_region_reduce") == 1 and prof.get("k_make_vols") == 1 and "k_atom_region" not in prof, prof
        assert_region_equal(large, want, cases.tiled(12000), w.top, "%s 12000 cut=%.3g" % (w.name, cut))
        assert np.array_equal(large[2][:8000], small[2]) and np.array_equal(large[3][:8000], small[3])
        for k, count in ((0, want["n_pos"]), (1, want["n_neg"])):
            assert np.all(np.abs(large[k][:8000] - small[k]) <= 1e-9 * count[cases.tiled(8000)] * w.top)


def test_region_sums_past_65536_groups(world):
    """70 000 atoms: k_sphere_paint x 1, k_region_reduce x 1 on a grid of 65536 blocks -- the blocks of atoms 0..4463 go on to atoms
    65536..69999 (other positions: 65536 % 3001 != 0); k_make_vols x 1 in 69 trips."""
    w = world
    for cut in (w.sigma, 0.1):
        got, prof = per_atom_region(w, 70000, cut)
        assert prof.get("k_sphere_paint") == 1 and prof.get("k_region_reduce") == 1 and prof.get("k_make_vols") == 1 and "k_atom_region" not in prof, prof
        assert not np.array_equal(cases.tiled(70000)[:4464], cases.tiled(70000)[65536:])
        assert_region_equal(got, region_want(w, cut), cases.tiled(70000), w.top, "%s 70000 cut=%.3g" % (w.name, cut))


# ---- 3: grouped region sums ----------------------------------------------------------------------------------------------------
def test_grouped_region_sums_past_the_staged_row(world):
    """24 000 atoms in 6 000 groups of 4 consecutive tiled positions (a row of 1.6 MB): k_init_bounds, k_atom_boxes, k_make_vols (6
    trips of 1024 groups, volumes of many sizes: a group's box spans its four spheres), k_sphere_paint, k_region_reduce x 1 each, no
    k_atom_region.  Radius 1.9 on the four atoms of 512 groups (every 11th from group 7), 0.7 elsewhere.  The checker computes all
    6 000 groups (nothing is expanded: the 0.7 A groups repeat with period 3001, the 1.9 A ones do not)."""
    from pdb_eda_amd import synthetic
    w = world
    n = 24000
    sizes = synthetic.draw_group_sizes(np.random.default_rng(5), n, choices=(4,))
    assert sizes == [4] * 6000
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xyz = w.base[cases.tiled(n)]
    rad = np.full(n, RADIUS, dtype=np.float32)
    for g in np.arange(512) * 11 + 7:
        rad[off[g]:off[g + 1]] = 1.9
    spheres = spheres_checker.atom_spheres(w.header, w.grid, xyz, rad, crs2xyz=w.dm._map.crs2xyz)
    every = np.arange(len(sizes))
    for cut in (w.sigma, 0.1):
        want = spheres_checker.region_sums(w.header, w.grid, xyz, rad, cut, group_offsets=off, spheres=spheres)
        per_atom = np.add.reduceat(np.diff(spheres["offsets"]), off[:-1])
        assert want["cnt"].sum() > 0 and 0 < want["n_pos"].sum() + want["n_neg"].sum() < want["cnt"].sum()
        assert 500 < np.count_nonzero(per_atom > want["cnt"]) < 5500          # groups whose spheres share voxels, and groups whose spheres do not
        assert want["valid"].any() and (w.name == "orth" or not want["valid"].all())
        got, prof = twice(w, lambda m: m.region_sums(xyz, rad, off, cut), same_arrays)
        assert prof.get("k_sphere_paint") == 1 and prof.get("k_region_reduce") == 1 and prof.get("k_make_vols") == 1 and "k_atom_region" not in prof, prof
        assert_region_equal(got, want, every, w.top, "%s grouped cut=%.3g" % (w.name, cut))


# ---- 4: per-atom blobs -----------------------------------------------------------------------------------------------------------
def voxel_keys(crs):
    crs = np.asarray(crs, dtype=np.int64).reshape(-1, 3)
    return ((crs[:, 0] + 4096) * 8192 + crs[:, 1] + 4096) * 8192 + crs[:, 2] + 4096


def blob_rows(bl):
    """The list's rows and its voxels, blob by blob; a blob's voxels sorted (the list is a set per blob: pdbeda_bloblist_voxels fixes
    the order of the blobs, not the order inside one)."""
    st = bl.stats()
    vox, voff = bl.voxels()
    out = {k: st[k] for k in ("n", "totalDensity", "group", "firstKey")}
    blob_of = np.repeat(np.arange(len(voff) - 1), np.diff(voff))
    out["vox"], out["voff"] = vox[np.lexsort((voxel_keys(vox), blob_of))], voff
    bl.free()
    return out


def blobs_want(w, cut):
    """Per position: the oracle's blobs as a sorted list of (the blob's sorted voxel keys as bytes, totalDensity)."""
    if ("blobs", cut) not in w.cache:
        rows = []
        for p in w.base:
            found = w.oracle.find_aberrant_blobs([p], [np.float32(RADIUS)], cut)
            rows.append(sorted((np.sort(voxel_keys(b["crs"])).tobytes(), float(b["totalDensity"])) for b in found))
        w.cache[("blobs", cut)] = rows
    return w.cache[("blobs", cut)]


def assert_blobs_equal(got, want, idx, top, what):
    n_blobs = len(got["n"])
    assert np.array_equal(np.diff(got["voff"]), got["n"]), what
    blob_of = np.repeat(np.arange(n_blobs), got["n"])
    key = voxel_keys(got["vox"])          # (sorted inside every blob: blob_rows)
    assert np.all((np.diff(key) > 0) | (np.diff(blob_of) > 0)), what
    mine = [[] for _ in idx]
    for r in range(n_blobs):
        mine[got["group"][r]].append((key[got["voff"][r]:got["voff"][r + 1]].tobytes(), float(got["totalDensity"][r])))
    worst, worst_bound, total = 0.0, 0.0, 0
    for g, rows in enumerate(mine):
        theirs = want[idx[g]]
        rows.sort()
        assert len(rows) == len(theirs), (what, g)
        for (a, x), (b, y) in zip(rows, theirs):
            assert a == b, (what, g)          # the same voxel set
            bound = 1e-9 * (len(a) // 8) * top
            assert abs(x - y) <= bound, (what, g, x, y)
            if abs(x - y) > worst:
                worst, worst_bound = abs(x - y), bound
            total += len(a) // 8
    print("%s: max |totalDensity - oracle| = %.3g (bound at that blob %.3g), %d voxels in %d blobs" % (what, worst, worst_bound, total, n_blobs))
    assert total > 0


def per_atom_blobs(w, n, cut):
    xyz = w.base[cases.tiled(n)]
    rad, off = np.full(n, RADIUS, dtype=np.float32), np.arange(n + 1, dtype=np.int64)
    return twice(w, lambda m: blob_rows(m.sphere_blobs(xyz, rad, off, cut)), same_arrays)


def test_sphere_blobs_below_and_above_the_staged_row(world):
    """8 000 atoms: k_atom_engine x 1 and k_emit x 1, no k_sphere_paint.  12 000 atoms: k_init_bounds, k_atom_boxes, k_make_vols,
    k_sphere_paint and the generic engine (k_run_index, k_union, k_resolve, k_paint_keys, k_emit), x 1 each, no k_atom_engine."""
    w = world
    for cut in (w.sigma, 0.0):
        want = blobs_want(w, cut)
        small, prof = per_atom_blobs(w, 8000, cut)
        assert prof.get("k_atom_engine") == 1 and "k_sphere_paint" not in prof, prof
        assert_blobs_equal(small, want, cases.tiled(8000), w.top, "%s blobs 8000 cut=%.3g" % (w.name, cut))
        large, prof = per_atom_blobs(w, 12000, cut)
        assert "k_atom_engine" not in prof and prof.get("k_sphere_paint") == 1 and prof.get("k_make_vols") == 1 and prof.get("k_union", 0) >= 1, prof
        assert_blobs_equal(large, want, cases.tiled(12000), w.top, "%s blobs 12000 cut=%.3g" % (w.name, cut))
        if cut == 0.0:          # every voxel of the sphere is in one of the atom's blobs
            cnt = region_want(w, 0.0)["cnt"]
            for got, n in ((small, 8000), (large, 12000)):
                assert np.array_equal(np.bincount(got["group"], weights=got["n"], minlength=n).astype(np.int64), cnt[cases.tiled(n)])


def test_sphere_blobs_past_65536_groups(world):
    """70 000 atoms at cutoff 0: k_init_bounds, k_atom_boxes, k_make_vols (69 trips), k_sphere_paint and the generic engine (k_run_index,
    k_union, k_resolve, k_paint_keys, k_emit), x 1 each; a group's blob sizes add up to
    region_sums' cnt, and the groups come 0..N-1 in order."""
    w = world
    n = 70000
    got, prof = per_atom_blobs(w, n, 0.0)
    assert "k_atom_engine" not in prof and prof.get("k_sphere_paint") == 1 and prof.get("k_make_vols") == 1, prof
    xyz = w.base[cases.tiled(n)]
    cnt = w.dm._map.region_sums(xyz, np.full(n, RADIUS, dtype=np.float32), np.arange(n + 1, dtype=np.int64), 0.0)[2]
    want = region_want(w, 0.0)["cnt"][cases.tiled(n)]
    assert want.min() > 0 and np.array_equal(cnt, want)
    assert np.array_equal(np.bincount(got["group"], weights=got["n"], minlength=n).astype(np.int64), cnt)
    assert np.all(np.diff(got["group"]) >= 0) and np.array_equal(np.unique(got["group"]), np.arange(n))
    assert np.array_equal(np.diff(got["voff"]), got["n"])


# ---- 5, 6: radial profiles ---------------------------------------------------------------------------------------------------------
def expanded(want, idx):
    return {k: v[idx] for k, v in want.items()}


def profiles_70000(w):
    """70 000 atoms, 2 shells, radius 0.7 at 1.5 sigma in the default mode: (arrays, kernels) -- shared by cases 5 and 6."""
    if "p70000" not in w.cache:
        xyz = w.base[cases.tiled(70000)]
        w.cache["p70000"] = twice(w, lambda m: m.radial_profiles(xyz, RADIUS, 2, w.sigma), same_arrays)
    return w.cache["p70000"]


def test_radial_profiles_across_chunks(world):
    """4 500 atoms x 64 shells, radius 1.0 (2 097 bytes of the pinned block an atom): k_atom_shells x 3, so rows are delivered at
    a0 > 0 twice.  The checker runs on the first 1001 positions (1001 = 7 x 11 x 13: coprime to the chunk sizes' powers of two) and is
    expanded.  Then 70 000 atoms x 2 shells, radius 0.7 (113 bytes an atom): k_atom_shells x 2."""
    w = world
    p = 1001
    idx = np.arange(4500) % p
    xyz = w.base[idx]
    for cut in (0.0, w.sigma):
        want = profiles_checker.radial_profiles(w.header, w.grid, w.base[:p], 1.0, 64, cut, crs2xyz=w.dm._map.crs2xyz)
        assert want["n"].sum() > 0 and (cut == 0.0 or 0 < want["n_sig"].sum() < want["n"].sum())
        assert want["valid"].any() and (w.name == "orth" or not want["valid"].all())
        got, prof = twice(w, lambda m: m.radial_profiles(xyz, 1.0, 64, cut), same_arrays)
        assert prof.get("k_atom_shells", 0) >= 2, prof
        assert_profiles_equal(got, expanded(want, idx), w.grid, "%s 4500 x 64 cut=%.3g" % (w.name, cut))
    got, prof = profiles_70000(w)
    assert prof.get("k_atom_shells", 0) >= 2, prof
    want = profiles_checker.radial_profiles(w.header, w.grid, w.base, RADIUS, 2, w.sigma, crs2xyz=w.dm._map.crs2xyz)
    assert 0 < want["n_sig"].sum() < want["n"].sum() and np.all(want["n"].sum(0) > 0)
    assert_profiles_equal(got, expanded(want, cases.tiled(70000)), w.grid, "%s 70000 x 2" % w.name)


SHELLS_WORKER = r'''
import io, json, sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
from pdb_eda_amd import _native, ccp4, synthetic
import batch_limit_cases as cases
ctx = _native.Context(0)
spec, grid = cases.spec_and_grid(%(name)r)
dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), %(name)r, ctx=ctx)
xyz = cases.base_atoms(%(name)r, dm.header)[cases.tiled(70000)]
cut = float(dm.meanDensity + 1.5 * dm.stdDensity)
ctx.profile_begin()
got = dm._map.radial_profiles(xyz, 0.7, 2, cut)
json.dump({k: v[0] for k, v in ctx.profile_end().items()}, open(%(prof)r, "w"))
np.savez(%(out)r, cut=cut, **got)
'''


def test_radial_profiles_grid_stride_without_copy_kernels(world, tmp_path):
    """PDBEDA_COPY_KERNELS=0 in a fresh process: 70 000 atoms x 2 shells are one chunk (8 MiB / 113 bytes), so k_atom_shells x 1
    on 65536 blocks, whose LDS shell tables serve atoms v and v + 65536.  The sums are folded as integers: the same bytes as the
    default mode's two launches."""
    w = world
    script, out, prof_path = tmp_path / "worker.py", tmp_path / "rows.npz", tmp_path / "prof.json"
    script.write_text(SHELLS_WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "name": w.name, "out": str(out), "prof": str(prof_path)})
    proc = subprocess.run([sys.executable, str(script)], env=dict(os.environ, PDBEDA_COPY_KERNELS="0"), capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-3000:]
    prof = json.loads(prof_path.read_text())
    print("%s: kernels %s" % (w.name, json.dumps(prof, sort_keys=True)))
    assert prof.get("k_atom_shells") == 1, prof
    z = np.load(str(out))
    assert float(z["cut"]) == w.sigma
    got = {k: z[k] for k in ("n", "sum", "nSig", "sumSig", "valid")}
    want = profiles_checker.radial_profiles(w.header, w.grid, w.base, RADIUS, 2, w.sigma, crs2xyz=w.dm._map.crs2xyz)
    idx = cases.tiled(70000)
    assert not np.array_equal(want["n"][idx[:4464]], want["n"][idx[65536:]])          # atoms v and v + 65536 fill their shells differently
    assert 0 < want["n_sig"].sum() < want["n"].sum()
    assert_profiles_equal(got, expanded(want, idx), w.grid, "%s 70000 x 2 without copy kernels" % w.name)
    default, _ = profiles_70000(w)
    for k in got:
        assert got[k].tobytes() == default[k].tobytes(), k
