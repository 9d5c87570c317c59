"""pdbeda_sphere_blobs, pdbeda_region_sums and pdbeda_aggregate_cloud refuse a non-finite coordinate with PDBEDA_ERR_ARGUMENT before
anything is staged or launched, and name the atom (include/pdbeda.h); the context goes on working.

8 atoms of radius 0.7 on the `orth` world of tests/batch_limit_cases.py, a NaN in the coordinates of atom 4.  After each refusal the
same context gives, for the 7 good atoms, what the yardsticks give: tests/spheres_checker.py (region sums, the bound of
tests/test_gpu_batch_limits.py), the oracle's find_aberrant_blobs (blobs) and tests/cloud_checker.py (aggregateCloud).  Then
Context.close() returns 0: nothing was left lent."""
import numpy as np
import pytest

import batch_limit_cases
import cloud_cases
import cloud_checker
import spheres_checker
from test_gpu_batch_limits import assert_blobs_equal, assert_region_equal, blob_rows, voxel_keys

pytestmark = pytest.mark.gpu

RADIUS = 0.7
BAD = 4


def test_a_nan_coordinate_is_refused_and_the_context_goes_on():
    from pdb_eda_amd import _native
    from oracle import oracle as ora
    spec, grid = batch_limit_cases.spec_and_grid("orth")
    header = cloud_cases.header_of(spec)
    xyz = batch_limit_cases.base_atoms("orth", header)[:8].copy()
    bad = xyz.copy()
    bad[BAD, 1] = np.nan
    good = np.delete(xyz, BAD, axis=0)
    g64 = grid.astype(np.float64)
    cut, top = float(np.float32(g64.mean() + 0.25 * g64.std())), float(np.abs(grid).max())
    oracle = ora.Oracle(header, grid)

    def entry(p):
        n = len(p)
        return cloud_cases.chain_entry(p, np.full(n, RADIUS, dtype=np.float32), 6.0 + 0.5 * np.arange(n), np.arange(n) // 4, cut, min_electrons=5.0)

    def batch(p):
        return p, np.full(len(p), RADIUS, dtype=np.float32), np.arange(len(p) + 1, dtype=np.int64)

    ctx = _native.Context(0)
    dm = cloud_cases.device_map(spec, grid, "refusals", ctx)
    m = dm._map
    every = np.arange(7)
    calls = {"sphere_blobs": lambda p: m.sphere_blobs(*batch(p), cut), "region_sums": lambda p: m.region_sums(*batch(p), cut),
             "aggregate_cloud": lambda p: cloud_cases.call(m, entry(p))}
    # the yardsticks' results for the 7 good atoms, once
    want_region = spheres_checker.region_sums(header, grid, good, RADIUS, cut, spheres=spheres_checker.atom_spheres(header, grid, good, RADIUS, crs2xyz=m.crs2xyz))
    assert want_region["cnt"].sum() > 0
    want_blobs = [sorted((np.sort(voxel_keys(b["crs"])).tobytes(), float(b["totalDensity"])) for b in oracle.find_aberrant_blobs([p], [np.float32(RADIUS)], cut)) for p in good]
    e = entry(good)
    clouds = cloud_checker.atom_clouds(oracle, e["xyz"], e["radius"], e["cutoff"])
    want_cloud = cloud_checker.aggregate_cloud(header, grid, clouds, *[e[k] for k in cloud_cases.ARGS if k != "radius"], e["min_electrons"])
    for name, call in calls.items():
        ctx.profile_begin()          # (the refused call's own profile: it launched nothing)
        try:
            with pytest.raises(_native.PdbedaError) as err:
                call(bad)
        finally:
            prof = ctx.profile_end()
        assert err.value.code == _native.PDBEDA_ERR_ARGUMENT and "atom %d " % BAD in str(err.value) and "non-finite" in str(err.value), (name, str(err.value))
        assert prof == {}, (name, prof)
        # the 7 good atoms on the same context, against the yardsticks
        assert_region_equal(m.region_sums(*batch(good), cut), want_region, every, top, "region sums after the refused " + name)
        assert_blobs_equal(blob_rows(m.sphere_blobs(*batch(good), cut)), want_blobs, every, top, "blobs after the refused " + name)
        got = cloud_cases.call(m, e)
        assert len(got["atom"]) > 0
        cloud_checker.assert_same_tables(got, want_cloud, what="aggregateCloud against the checker after the refused " + name)
        cloud_checker.assert_same_tables(got, cloud_cases.call(oracle, e), what="aggregateCloud against the oracle after the refused " + name)
    dm._map.free()
    assert ctx.close() == 0
