"""The blob shape call (pdbeda_bloblist_moments) against the only route to the same sums the library had before it:
DeviceBlobs.voxelLists() (12 B per voxel to the host), pdbeda_point_density of those voxels (up and down again) and numpy segment
sums (add / minimum / maximum .reduceat) -- kept here as the comparison.  256^3 smooth noise, the fused green / red lists of one
labelling call, two workloads:

  sigma_1.5   +-1.5 sigma: about a million voxels per list, thousands of blobs;
  sigma_3     +-3 sigma: the lists of the difference-map analysis.

Every repetition labels the map afresh (a list keeps its rows: a second call on the same list would time a copy) and materialises the
voxel lists on the device before anything is timed, for both routes; a repetition runs both routes, the device call first on one pair of
lists, the host route on another.  Medians after warm-up, one JSON line per workload.  --only-moments leaves the host route out (a
profiler run of the new kernels).  The figures are written into DESIGN.md 4.8."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"sigma_1.5": 1.5, "sigma_3": 3.0}
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def host_route(bl, device_map, parts):
    """The sums of pdbeda_bloblist_moments from the voxel lists on the host; parts: seconds by phase, added to."""
    t0 = time.perf_counter()
    crs, off = bl.voxels()
    t1 = time.perf_counter()
    rho = device_map.point_density(crs)
    t2 = time.perf_counter()
    out = None
    if len(off) > 1:
        starts = off[:-1]
        blob = np.repeat(np.arange(len(starts)), np.diff(off))
        lo, hi = np.minimum.reduceat(crs, starts, axis=0), np.maximum.reduceat(crs, starts, axis=0)
        w = np.abs(rho)
        top = np.maximum.reduceat(w, starts)
        tied = np.nonzero(w == top[blob])[0]
        order = tied[np.lexsort((crs[tied, 2], crs[tied, 1], crs[tied, 0], blob[tied]))]          # by blob, then (c, r, s)
        first = order[np.concatenate([[True], blob[order][1:] != blob[order][:-1]])]
        d = (crs - lo[blob]).astype(np.int64)
        dd = np.stack([d[:, i] * d[:, j] for i, j in PAIRS], axis=1)
        out = {"boxLo": lo, "boxHi": hi, "extremeCrs": crs[first], "extreme": rho[first].astype(np.float32), "s1": np.add.reduceat(d, starts, axis=0),
               "s2": np.add.reduceat(dd, starts, axis=0), "sw": np.add.reduceat(w, starts), "sw1": np.add.reduceat(w[:, None] * d, starts, axis=0),
               "sw2": np.add.reduceat(w[:, None] * dd, starts, axis=0)}
    t3 = time.perf_counter()
    for k, v in (("download", t1 - t0), ("point_density", t2 - t1), ("numpy", t3 - t2)):
        parts[k] = parts.get(k, 0.0) + v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--workloads", default="sigma_1.5,sigma_3")
    ap.add_argument("--only-moments", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    ctx = _native.default_context()
    spec = synthetic.MapSpec(ncrs=(args.grid,) * 3, spacing=0.4)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=1, sigma_voxels=1.5))), "noise", ctx=ctx)

    def fresh(cut):
        """Both lists of one fused labelling call, their voxel lists made on the device (nothing comes to the host)."""
        lists = dm._map.full_blobs_pm(cut, -cut)
        for bl in lists:
            assert ctx._lib.pdbeda_bloblist_num_voxels(bl._h) >= 0
        ctx.synchronize()
        return lists

    for name in args.workloads.split(","):
        cut = dm.meanDensity + WORKLOADS[name] * dm.stdDensity
        times = {"moments": [], "host_route": [], "host_download": [], "host_point_density": [], "host_numpy": []}
        got = old = None
        for rep in range(args.warmup + args.reps):
            lists = fresh(cut)
            t0 = time.perf_counter()
            got = [bl.moments() for bl in lists]
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times["moments"].append(dt)
            if args.only_moments:
                continue
            lists = fresh(cut)
            parts = {}
            t0 = time.perf_counter()
            old = [host_route(bl, dm._map, parts) for bl in lists]
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times["host_route"].append(dt)
                for k, v in parts.items():
                    times["host_" + k].append(v)
        same = None
        if old is not None:
            same = all(o is None or all(np.array_equal(g[k], o[k]) for k in ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2")) for g, o in zip(got, old))
        lists = fresh(cut)
        sizes = np.concatenate([bl.stats()["n"] for bl in lists])
        ctx.profile_begin()
        for bl in lists:
            bl.moments()
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        out = {"workload": name, "grid": [args.grid] * 3, "cutoff_sigma": WORKLOADS[name], "lists": 2, "blobs": int(len(sizes)), "voxels": int(sizes.sum()),
               "largest_blob": int(sizes.max(initial=0)), "reps": args.reps, "warmup": args.warmup, "median_ms": med,
               "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "kernel_ms": prof, "integer_columns_equal": same,
               "ratio_host_route_over_moments": round(med["host_route"] / med["moments"], 1) if "host_route" in med else None}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
