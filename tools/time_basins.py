"""Peak basins: time of one whole call (peak search, list order, basins; synchronised, after warm-up) for the fused 3 sigma lists
and the 1.5 sigma list of a 256^3 synthetic map (smooth noise, the generator of the bench), with and without the basin volume, beside
the peak search alone; the kernels (HIP events on the context's stream) separately -- k_peak_stencil makes the same tile pass over the
same map as k_basin_parent and is the yardstick in the same run.  The host route a user has without the feature is timed by this
tool's own numpy code: the grid to the host, a steepest ascent over the significant voxels, counts and sums per root.
    python tools/time_basins.py [--edge 256] [--reps 20] [--out FILE]
Prints one JSON document.  Under `rocprofv3 --kernel-trace --stats -- python tools/time_basins.py` the kernel times are the tool's."""
import argparse
import io
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, call, reps):
    """Median / min wall time of call() (which must end synchronised), and the per-kernel means of one profiled repetition set."""
    for _ in range(2):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
    ctx.profile_begin()
    for _ in range(reps):
        call()
    prof = ctx.profile_end()
    return {"call_ms_median": round(1e3 * float(np.median(wall)), 4), "call_ms_min": round(1e3 * float(np.min(wall)), 4),
            "per_call_us": {name: round(1e3 * ms / reps, 2) for name, (calls, ms) in sorted(prof.items())},
            "launches_per_call": {name: calls / reps for name, (calls, ms) in sorted(prof.items())}}


def host_route(device_map, cutoff):
    """What a user does today: the grid to the host, then numpy.  Returns (seconds, basins, significant voxels)."""
    t0 = time.perf_counter()
    grid = device_map.download()                                   # [s][r][c]
    sig = grid >= np.float32(cutoff)
    mag = np.where(sig, grid, np.float32(0))
    # descending value, ties by c-major position: the order of the peak search
    us, ur, uc = grid.shape
    s, r, c = np.nonzero(sig)
    position = (c.astype(np.int64) * ur + r) * us + s
    order = np.lexsort((position, -mag[s, r, c].astype(np.float64)))
    rank = np.full((us + 2, ur + 2, uc + 2), len(order), dtype=np.int64)
    rank[s[order] + 1, r[order] + 1, c[order] + 1] = np.arange(len(order))
    best = rank[s + 1, r + 1, c + 1].copy()
    for ds, dr, dc in itertools.product((0, 1, 2), repeat=3):
        np.minimum(best, rank[s + ds, r + dr, c + dc], out=best)
    parent = order[best]                                           # rank -> index in the nonzero() enumeration of the significant voxels
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent = nxt
    roots, slot = np.unique(parent, return_inverse=True)
    n = np.bincount(slot)
    total = np.bincount(slot, weights=grid[s, r, c].astype(np.float64))
    assert len(n) == len(total)
    return time.perf_counter() - t0, len(roots), len(order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    ctx = _native.default_context()
    spec = synthetic.MapSpec(ncrs=(a.edge,) * 3, spacing=0.5)
    grid = synthetic.noise_grid(spec, seed=1, sigma_voxels=1.5)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "basins", ctx=ctx)
    mean, std = dm.meanDensity, dm.stdDensity
    out = {"edge": a.edge, "voxels": a.edge ** 3, "grid_bytes": 4 * a.edge ** 3, "reps": a.reps, "rows": []}
    c3, c15 = mean + 3 * std, mean + 1.5 * std

    def whole(lists, basins, volume):
        for pl in lists:
            pl.rows()
            if basins:
                pl.basins(volume=volume)
            pl.free()

    cases = []
    for name, make in (("fused 3 sigma lists", lambda: dm._map.peaks_pm(c3, -c3)), ("1.5 sigma list", lambda: [dm._map.peaks(c15)])):
        cases.append((name + ": peak search alone", make, False, False))
        cases.append((name + ": peak search + basins", make, True, False))
        cases.append((name + ": peak search + basins + volume", make, True, True))
    alone = None
    for name, make, basins, volume in cases:
        row = {"case": name}
        row.update(timed(ctx, lambda: whole(make(), basins, volume), a.reps))
        if not basins:
            alone = row["call_ms_median"]
        else:
            row["basins_ms_median_beyond_peak_search"] = round(row["call_ms_median"] - alone, 4)
            lists = make()
            got = [pl.basins() for pl in lists]
            row["peaks"] = [len(pl) for pl in lists]
            row["counters"] = [g["counters"] for g in got]
            row["basins_with_a_neighbour"] = [int((g["neighbour"] >= 0).sum()) for g in got]
            stencil, parent = row["per_call_us"].get("k_peak_stencil"), row["per_call_us"].get("k_basin_parent")
            if stencil and parent:
                row["k_basin_parent_over_k_peak_stencil"] = round(parent / stencil, 2)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    seconds, basins, significant = host_route(dm._map, c15)
    device = [r for r in out["rows"] if r["case"] == "1.5 sigma list: peak search + basins"][0]
    out["host_route"] = {"case": "1.5 sigma list: grid to the host + numpy steepest ascent (counts and sums only; one run)", "seconds": round(seconds, 3),
                         "basins": basins, "significant": significant,
                         "over_device_whole_call": round(1e3 * seconds / device["call_ms_median"], 1),
                         "device_includes": "peak search, list order on the host, basins with centres and saddles, rows to the host; the map is resident",
                         "host_includes": "the grid's copy to the host, ranking, parents, doubling, counts and sums; no centres, no saddles"}
    assert basins == device["peaks"][0] and significant == device["counters"][0]["significant"]
    text = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
