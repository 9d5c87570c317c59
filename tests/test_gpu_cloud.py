"""pdbeda_aggregate_cloud where no protein-like entry takes it (inputs: tests/cloud_cases.py, all of them checked on the CPU by
tests/test_cloud_host.py):

1. prefixes of a 48 000-atom entry on either side of the three sizes at which the call changes path -- the clouds' table in one trip
   (T1), the aux block staged for k_job_init (T2), the union job finished by k_union_finish (T3): tests/test_cloud_host.py, switch_points() --
   against the oracle composite, every row of every table; each call is repeated under the profiler on a context of its own, must
   give the same bytes, and T3's side shows in the kernel names;
2. 400 atoms that start 4 voxels outside the stored box, on a map whose whole cell is stored and on a triclinic one that stores part of
   it, against tests/cloud_checker.py and the oracle; the same atoms with about ten clouds each (more than the 4 n + 64 rows the first
   trip asks for), and an ordinary call on the same context after it;
3. a handful of atoms per decision rule on a map of dyadic densities: tables equal with ==.

Tolerances: cloud_checker.assert_same_tables."""
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

from conftest import ROOT
import batch_limit_cases
import cloud_cases as cases
import cloud_checker as checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prof_ctx():
    from pdb_eda_amd import _native
    return _native.Context(0)


def oracle_of(header, grid):
    from oracle import oracle as ora
    return ora.Oracle(header, grid)


def flat(result):
    out = {}
    for k, v in result.items():
        if isinstance(v, dict):
            out.update({k + "." + f: np.asarray(x) for f, x in v.items()})
        else:
            out[k] = np.asarray(v)
    return out


def assert_same_bytes(a, b):
    a, b = flat(a), flat(b)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def profiled(ctx, call):
    ctx.profile_begin()
    try:
        result = call()
    finally:
        prof = {k: v[0] for k, v in ctx.profile_end().items()}
    return result, prof


def checked(header, grid, oracle, e):
    clouds = checker.atom_clouds(oracle, e["xyz"], e["radius"], e["cutoff"])
    return checker.aggregate_cloud(header, grid, clouds, *[e[k] for k in cases.ARGS if k != "radius"], e["min_electrons"])


# ---- 1. the large entry across T1-T3 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(gpu_ctx, prof_ctx):
    t0 = time.perf_counter()
    spec, header, grid, e = cases.big_entry()
    oracle = oracle_of(header, grid)
    b = types.SimpleNamespace(spec=spec, grid=grid, entry={n: cases.prefix(e, n) for n in cases.BIG_SIZES})
    b.want = {n: cases.call(oracle, p) for n, p in b.entry.items()}
    print("large entry: map, atoms and the oracle's tables of %d sizes in %.1f s on the host" % (len(cases.BIG_SIZES), time.perf_counter() - t0))
    b.dm = cases.device_map(spec, grid, "big", gpu_ctx)
    b.dm_prof = cases.device_map(spec, grid, "big", prof_ctx)
    b.got = {}
    return b


def big_call(b, n):
    if n not in b.got:
        b.got[n] = cases.call(b.dm._map, b.entry[n])
    return b.got[n]


@pytest.mark.parametrize("n", cases.BIG_SIZES)
def test_large_entry_against_the_oracle(big, prof_ctx, n):
    """Sizes 11 000 (below T2, T1 and T3), 19 000 (above T2), 29 000 (above T2 and T1), 48 000 (above all): every row of every table
    against the oracle's; the same bytes from a second call under the profiler; k_pool_paint x 1, and k_union_finish x 1 without
    k_pool_component below T3, k_pool_component x 1 without k_union_finish above it."""
    got, want = big_call(big, n), big.want[n]
    checker.assert_same_tables(got, want, ordered=False, what="%d atoms" % n)
    assert np.array_equal(got["res"]["residue"], want["res"]["residue"])          # (residue by residue, as the ABI fixes it)
    again, prof = profiled(prof_ctx, lambda: cases.call(big.dm_prof._map, big.entry[n]))
    print("%d atoms: kernels %s" % (n, json.dumps(prof, sort_keys=True)))
    assert_same_bytes(got, again)
    assert prof.get("k_pool_paint") == 1 and "k_pool_gather" not in prof and "k_test_overlap" not in prof, prof
    if n == cases.BIG_SIZES[-1]:
        assert prof.get("k_pool_component") == 1 and "k_union_finish" not in prof, prof
    else:
        assert prof.get("k_union_finish") == 1 and "k_pool_component" not in prof, prof


CLOUD_WORKER = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
from pdb_eda_amd import _native, synthetic
import cloud_cases as cases
z = np.load(%(inputs)r)
ctx = _native.Context(0)
dm = cases.device_map(synthetic.MapSpec(ncrs=z["grid"].shape[::-1], spacing=0.5), z["grid"], "child", ctx)
e = {k: z[k] for k in cases.ARGS}
e.update(cutoff=float(z["cutoff"]), min_electrons=float(z["min_electrons"]))
ctx.profile_begin()
got = cases.call(dm._map, e)
prof = ctx.profile_end()
flat = {"kernels": np.array(sorted(prof))}
for k, v in got.items():
    if isinstance(v, dict):
        flat.update({k + "." + f: x for f, x in v.items()})
    else:
        flat[k] = np.asarray(v)
np.savez(%(out)r, **flat)
'''


@pytest.mark.parametrize("switch", ["PDBEDA_UNORDERED_UNION", "PDBEDA_COPY_KERNELS"])
def test_smallest_size_with_a_path_switched_off(big, tmp_path, switch):
    """The 11 000-atom prefix in a fresh process with PDBEDA_UNORDERED_UNION=0 (the ordered union job: k_pool_component) and with
    PDBEDA_COPY_KERNELS=0 (no kernel touches host memory: nothing staged for k_job_init, no k_union_finish): the parent's bytes in
    every table whose order the ABI fixes, the same multiset of domain rows."""
    n = cases.BIG_SIZES[0]
    got = flat(big_call(big, n))
    inputs, out, script = tmp_path / "inputs.npz", tmp_path / "tables.npz", tmp_path / "worker.py"
    np.savez(str(inputs), grid=big.grid, **big.entry[n])
    script.write_text(CLOUD_WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "inputs": str(inputs), "out": str(out)})
    proc = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-3000:]
    z = np.load(str(out))
    kernels = set(str(k) for k in z["kernels"])
    print("%s=0: kernels %s" % (switch, sorted(kernels)))
    assert "k_pool_component" in kernels and "k_union_finish" not in kernels and "k_pool_paint" in kernels
    for k, v in got.items():
        if not k.startswith("dom."):
            assert z[k].dtype == v.dtype and z[k].tobytes() == v.tobytes(), k
    order = lambda t: np.lexsort((t["dom.electrons"], t["dom.total"], t["dom.n"]))
    mine, theirs = order(got), order(z)
    for f in ("residue", "total", "n", "electrons", "centroid"):
        assert z["dom." + f][theirs].tobytes() == got["dom." + f][mine].tobytes(), f


# ---- 2. atoms that leave the stored box; many clouds an atom ----------------------------------------------------------------------
@pytest.fixture(scope="module", params=batch_limit_cases.WORLDS)
def world(request, gpu_ctx):
    w = types.SimpleNamespace(name=request.param)
    for kind in ("smooth", "noise"):
        spec, header, grid, e = cases.world_entry(w.name, kind)
        oracle = oracle_of(header, grid)
        setattr(w, kind, types.SimpleNamespace(entry=e, dm=cases.device_map(spec, grid, w.name + kind, gpu_ctx), oracle=cases.call(oracle, e),
                                               checker=checked(header, grid, oracle, e)))
    return w


def test_atoms_outside_the_stored_box(world):
    """Spheres with raw crs below zero, wrapped density on the full cell (orth), zero density beyond what is stored (skew), union
    volumes whose origin is negative."""
    s = world.smooth
    got = cases.call(s.dm._map, s.entry)
    checker.assert_same_tables(got, s.oracle, what=world.name + " against the oracle")
    checker.assert_same_tables(got, s.checker, what=world.name + " against the checker")


def test_more_clouds_than_the_first_trip_asks_for(world):
    """About ten clouds an atom (4 144 / 4 200 clouds of 400 atoms against 4 n + 64 = 1 664 rows): the table comes by the two-step
    path.  Then an ordinary call on the same context: the pinned block and the context are as sound as before."""
    s = world.noise
    got = cases.call(s.dm._map, s.entry)
    checker.assert_same_tables(got, s.oracle, what=world.name + " noise against the oracle")
    checker.assert_same_tables(got, s.checker, what=world.name + " noise against the checker")
    after = cases.call(world.smooth.dm._map, world.smooth.entry)
    checker.assert_same_tables(after, world.smooth.oracle, what=world.name + " after the fallback")
    assert_same_bytes(cases.call(s.dm._map, s.entry), got)


# ---- 3. crafted decision cases -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted(gpu_ctx, prof_ctx):
    spec, header, grid, entries = cases.crafted()
    c = types.SimpleNamespace(header=header, grid=grid, entries=entries, oracle=oracle_of(header, grid))
    c.dm = cases.device_map(spec, grid, "crafted", gpu_ctx)
    c.dm_prof = cases.device_map(spec, grid, "crafted", prof_ctx)
    return c


@pytest.mark.parametrize("name", ["equidistant", "cutoff", "threshold", "corner", "chain", "ordinals", "aliases", "no_pairs", "nothing", "empty"])
def test_decision_case(crafted, name):
    """What each case pins is asserted on the oracle's tables by tests/test_cloud_host.py; here the device's tables equal the oracle's
    and the checker's with == (centroids and distances at 1e-12).  After the cases that leave early (nothing pooled, no atoms) a
    normal call on the same context is correct."""
    c, e = crafted, crafted.entries[name]
    got = cases.call(c.dm._map, e)
    checker.assert_same_tables(got, cases.call(c.oracle, e), exact=True, what=name + " against the oracle")
    checker.assert_same_tables(got, checked(c.header, c.grid, c.oracle, e), exact=True, what=name + " against the checker")
    if name in ("nothing", "empty"):
        assert len(got["atom"]) == 0 and np.isnan(got["centroidDistanceCutoff"]) and not got["owner_state"].any()
        e = c.entries["chain"]
        checker.assert_same_tables(cases.call(c.dm._map, e), cases.call(c.oracle, e), exact=True, what="chain after " + name)


def test_refusals(crafted, prof_ctx):
    """PDBEDA_ERR_ARGUMENT for an alias, a key, an owner key out of range and for decreasing residues before anything is launched; for a
    bonded key out of range after the clouds' job (it is found when its owner's pairs are listed) and before the union job.  A correct
    call follows each on the same context."""
    from pdb_eda_amd import _native
    c, e = crafted, crafted.entries["chain"]
    want = cases.call(c.oracle, e)
    for what, bad in cases.refusals(e).items():
        prof_ctx.profile_begin()          # (the refused call's own profile: what it launched before it returned)
        try:
            with pytest.raises(_native.PdbedaError) as err:
                cases.call(c.dm_prof._map, bad)
        finally:
            prof = prof_ctx.profile_end()
        assert err.value.code == _native.PDBEDA_ERR_ARGUMENT, what
        if what == "bonded key out of range":
            assert "k_pool_paint" not in prof and "k_union_finish" not in prof, (what, prof)
        else:
            assert prof == {}, (what, prof)
        checker.assert_same_tables(cases.call(c.dm_prof._map, e), want, exact=True, what="after " + what)
