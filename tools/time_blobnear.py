"""The nearest-blob call (pdbeda_bloblist_nearest) against the route it replaces: labels() of the other list and voxelLists() of this one
to the host, then scipy -- either a cKDTree of the other list's voxel centres queried with this list's, or a Euclidean distance
transform of the other list's mask sampled at this list's voxels; both are timed, the quicker one is the host route and is named in the
output.  256^3 smooth noise, the fused green / red lists of one labelling call, BOTH directions (green -> red and red -> green), a table
to 2.5 A, two workloads:

  sigma_1.5   +-1.5 sigma: about a million voxels per list, thousands of blobs;
  sigma_3     +-3 sigma: the lists of the difference-map analysis.

Every repetition labels the map afresh and materialises the voxel lists on the device before anything is timed, for both routes.  The
host route gives a distance per blob (the minimum over its voxels, NaN beyond the reach); the tool checks that it agrees with the
distance of the device call's table entry, and fails when it does not.  Medians after warm-up, one JSON line per workload and the whole result in --out.  The
figures are written into DESIGN.md 4.9."""
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


def host_gap(a, b, shape, step, reach, how, parts):
    """Per blob of ``a`` the distance (A) to the nearest voxel of ``b``, NaN beyond ``reach``: the host route.  An orthogonal grid; step: A per voxel along c, r, s."""
    t0 = time.perf_counter()
    crs, off = a.voxels()
    labels = b.labels(shape)
    t1 = time.perf_counter()
    gap = np.full(len(off) - 1, np.nan)
    if len(crs) and (labels >= 0).any():
        if how == "edt":
            from scipy import ndimage
            d = ndimage.distance_transform_edt(labels < 0, sampling=step[::-1])[crs[:, 2], crs[:, 1], crs[:, 0]]
        else:
            from scipy.spatial import cKDTree
            s, r, c = np.nonzero(labels >= 0)
            tree = cKDTree(np.stack([c, r, s], axis=1) * step)
            d, _ = tree.query(crs * step, k=1, distance_upper_bound=reach * (1.0 + 1e-9))
        gap = np.minimum.reduceat(d, off[:-1])
        gap[~(gap <= reach * (1.0 + 1e-9))] = np.nan
    t2 = time.perf_counter()
    parts["download"] = parts.get("download", 0.0) + (t1 - t0)
    parts["scipy"] = parts.get("scipy", 0.0) + (t2 - t1)
    return gap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reach", type=float, default=2.5)
    ap.add_argument("--workloads", default="sigma_1.5,sigma_3")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_blobnear_time.json"))
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    ctx = _native.default_context()
    spec = synthetic.MapSpec(ncrs=(args.grid,) * 3, spacing=0.4)
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=1, sigma_voxels=1.5))), "noise", ctx=ctx)
    table, distance = ccp4.neighbourOffsets(dm.header, args.reach)
    assert dm.header.orthogonal
    # (the header's own steps: its cell edges are float32, so 256 voxels of 0.4 A are 6e-9 A longer each than 0.4)
    step = np.linalg.norm(dm.header.crs2xyz_array(np.eye(3)) - dm.header.crs2xyz_array(np.zeros((1, 3))), axis=1)
    shape = dm._map.unique_shape

    def fresh(cut):
        """Both lists of one fused labelling call, their voxel lists made on the device (nothing comes to the host)."""
        lists = dm._map.full_blobs_pm(cut, -cut)
        for bl in lists:
            assert ctx._lib.pdbeda_bloblist_num_voxels(bl._h) >= 0
        ctx.synchronize()
        return lists

    results = []
    for name in args.workloads.split(","):
        cut = dm.meanDensity + WORKLOADS[name] * dm.stdDensity
        times = {"nearest": [], "host_kdtree": [], "host_kdtree_download": [], "host_kdtree_scipy": [], "host_edt": [], "host_edt_download": [], "host_edt_scipy": []}
        got, gaps = None, {}
        for rep in range(args.warmup + args.reps):
            green, red = fresh(cut)
            t0 = time.perf_counter()
            got = [green.nearest(red, table), red.nearest(green, table)]
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times["nearest"].append(dt)
            if args.only_device:
                continue
            for how in ("kdtree", "edt"):
                green, red = fresh(cut)
                parts = {}
                t0 = time.perf_counter()
                gaps[how] = [host_gap(green, red, shape, step, args.reach, how, parts), host_gap(red, green, shape, step, args.reach, how, parts)]
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    times["host_" + how].append(dt)
                    for k, v in parts.items():
                        times["host_%s_%s" % (how, k)].append(v)
        agree = None
        if gaps:
            agree = True
            for how, both in gaps.items():
                for cols, gap in zip(got, both):
                    found = cols["index"] >= 0
                    agree = agree and bool(np.array_equal(found, ~np.isnan(gap)) and np.allclose(distance[cols["index"][found]], gap[found], rtol=0, atol=1e-9))
        assert agree is not False, "%s: the distances of the device call and of the host routes disagree" % name
        green, red = fresh(cut)
        sizes = [bl.stats()["n"] for bl in (green, red)]
        ctx.profile_begin()
        last = [green.nearest(red, table), red.nearest(green, table)]
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        quicker = None if args.only_device else min(("kdtree", "edt"), key=lambda how: med["host_" + how])
        out = {"workload": name, "grid": [args.grid] * 3, "cutoff_sigma": WORKLOADS[name], "reach_A": args.reach, "offsets": int(len(table)), "directions": 2,
               "blobs": [int(len(n)) for n in sizes], "voxels": [int(n.sum()) for n in sizes], "largest_blob": [int(n.max(initial=0)) for n in sizes],
               "with_partner": [int((cols["index"] >= 0).sum()) for cols in last], "largest_index": [int(cols["index"].max(initial=-1)) for cols in last],
               "reps": args.reps, "warmup": args.warmup, "median_ms": med, "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "kernel_ms": prof,
               "host_route": quicker, "distances_agree": agree,
               "ratio_host_route_over_nearest": round(med["host_" + quicker] / med["nearest"], 1) if quicker else None}
        print(json.dumps(out), flush=True)
        results.append(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(out) + "\n" for out in results))


if __name__ == "__main__":
    main()
