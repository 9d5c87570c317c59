"""The nearest-atom partition (pdbeda_map_partition) against the only route to the same owners the library had before it:
pdbeda_crs2xyz of every voxel of the box, pdbeda_nearest_atom (brute force, voxels x atoms) and a host bincount -- which gives
the owners and the voxel counts only, none of the density columns.  Two workloads, both at maxDistance 3.5 over the Fo-Fc map
and the symmetry atoms of the entry:

  bench_256     a 256^3 map (the size of bench.py's flagship map) with a 5 000-atom synthetic entry;
  analysis_128  bench.py's analysis entry: 128^3, 2 000 atoms.

All forms run in this process, interleaved (a repetition runs every form once); medians after warm-up.  The old route is timed
twice over: `old_route` is all of it (the crs triples made on the host, the two device calls per slab, the distance test and the
bincount), `old_route_device_calls` only the time spent inside pdbeda_crs2xyz and pdbeda_nearest_atom (copies included).
--only-partition leaves the old route out (a profiler run of the new kernels).  The figures are written into DESIGN.md 4.7."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"bench_256": ((256, 256, 256), 1000, 5, 0.5), "analysis_128": ((128, 128, 128), 400, 5, 0.5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--old-reps", type=int, default=2, help="repetitions of the old route (it takes seconds on the large map)")
    ap.add_argument("--workloads", default="analysis_128,bench_256")
    ap.add_argument("--only-partition", action="store_true")
    ap.add_argument("--max-distance", type=float, default=3.5)
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic, structure, densityAnalysis as da
    ctx = _native.default_context()
    for name in args.workloads.split(","):
        ncrs, n_res, seed, spacing = WORKLOADS[name]
        spec, header, st, params, dens, diff, rot = synthetic.cube_entry(ncrs, n_res, seed, spacing)
        da.setGlobals(params)
        densityObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), "synth", ctx=ctx)
        diffObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), "synth", ctx=ctx)
        da._attachCutoffs(densityObj, diffObj)
        an = da.DensityAnalysis("synth", densityObj, diffObj, st, structure.PDBEntry(structure.PDBHeader(pdbid="synth", resolution=2.0, spaceGroup="P_1", rotationMats=rot)))
        xyz = np.ascontiguousarray(an.symmetryAtomCoords, dtype=np.float64)
        cut = diffObj.meanDensity + 3.0 * diffObj.stdDensity
        us, ur, uc = diffObj._map.unique_shape
        maxd = float(np.float32(args.max_distance))

        def staged(owners=True):
            return diffObj._map.partition(xyz, args.max_distance, cut, owners=owners)

        def old_route():
            owner = np.empty(us * ur * uc, dtype=np.int32)
            inside[0] = 0.0
            plane = np.stack(np.meshgrid(np.arange(ur), np.arange(uc), indexing="ij"), axis=-1).reshape(-1, 2)
            step = max(1, (1 << 21) // len(plane))          # (slabs of about 2 M voxels: the coordinates of all of them would be 400 MB on the large map)
            for s0 in range(0, us, step):
                s1 = min(us, s0 + step)
                crs = np.empty(((s1 - s0) * len(plane), 3), dtype=np.int32)
                crs[:, 0], crs[:, 1] = np.tile(plane[:, 1], s1 - s0), np.tile(plane[:, 0], s1 - s0)
                crs[:, 2] = np.repeat(np.arange(s0, s1), len(plane))
                t0 = time.perf_counter()
                idx, dist = ctx.nearest_atom(diffObj._map.crs2xyz(crs), xyz)
                inside[0] += time.perf_counter() - t0
                owner[s0 * len(plane):s1 * len(plane)] = np.where(dist <= maxd, idx, -1)
            return owner, np.bincount(owner[owner >= 0], minlength=len(xyz))

        inside = [0.0]
        forms = {"partition": staged, "partition_no_owner_volume": lambda: staged(False)}
        times = {k: [] for k in list(forms) + ["old_route", "old_route_device_calls"]}
        for rep in range(args.warmup + args.reps):
            for k, fn in forms.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                if rep >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        got = staged()
        same = None
        if not args.only_partition:
            for rep in range(args.old_reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                old_owner, old_n = old_route()
                times["old_route"].append(time.perf_counter() - t0)
                times["old_route_device_calls"].append(inside[0])
            same = bool(np.array_equal(old_owner.reshape(got["owner"].shape), got["owner"]) and np.array_equal(old_n, got["n"]))
        ctx.profile_begin()
        staged()
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        out = {"workload": name, "grid": list(ncrs), "atoms": len(list(st.get_atoms())), "symmetry_atoms": len(xyz), "max_distance": args.max_distance,
               "reps": args.reps, "old_reps": len(times["old_route"]), "median_ms": med, "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v},
               "kernel_ms": prof, "old_route_owners_equal": same,
               "ratio_old_over_partition": round(med["old_route"] / med["partition"], 1) if "old_route" in med else None,
               "ratio_old_device_calls_over_partition": round(med["old_route_device_calls"] / med["partition"], 1) if "old_route" in med else None,
               "owned_voxels": int(got["n"].sum()), "unowned_voxels": int(got["unownedN"][0])}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
