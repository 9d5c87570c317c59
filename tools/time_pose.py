"""The rigid-fragment pose search (pdbeda_pose_scores) against the only route the library offered before it: the coordinates of every atom of
every pose made on the host, pushed through `pdbeda_interp_density`, and the values reduced in numpy.  Two workloads:

  analysis_128  the Fo-Fc map of bench.py's analysis entry (128^3, 0.5 A): 500 centres x 4 096 rotations x a 20-atom fragment (radius 4 A);
  bench_256     a 256^3 noise map (the size of bench.py's flagship map): 2 000 centres x 4 096 rotations x a 40-atom fragment (radius 5 A).

One `DensityMatrix.poseScores(topK=5)` call per repetition, ended by the call's own wait; medians after warm-up.  The kernel by HIP events in
calls of their own (the context's profiler), staged and with staging switched off (PDBEDA_POSE_GLOBAL_ONLY).  The host route is timed on a
SLICE of --route-centres centres (all rotations, all atoms) and reported per pose beside the device's; the estimate for the whole workload is
the slice's time scaled by the number of centres and is marked as such.  The route's scores are compared with the call's on the slice (the
host's positions come from a plain einsum, not the fused dot product: they agree to rounding, not to the bit).  The host-to-device copy rate
of the same run -- the upload of the workload's map -- is printed beside them.  The figures are written into DESIGN.md 4.19."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fragment(n, radius, seed):
    """``n`` atoms in the ball of ``radius`` at bond-like spacing is not needed for a timing: seeded points, one of them on the sphere."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    x = u / np.linalg.norm(u, axis=1)[:, None] * (radius * np.cbrt(rng.uniform(0.0, 1.0, size=n)))[:, None]
    x[0] = [radius, 0.0, 0.0]
    return x, rng.uniform(1.0, 8.0, size=n)


def host_route(dm, frag, w, rot, centres, floor):
    """(scores, low, valid) [centres][rot] the way a caller had to spell it: coordinates up, values back, a reduction in numpy."""
    p = centres[:, None, None, :] + np.einsum("rij,aj->rai", rot, frag)[None, :, :, :]
    values, valid = dm._map.interp_density(p.reshape(-1, 3))
    values, valid = values.reshape(p.shape[:3]), valid.reshape(p.shape[:3])
    return (values * w[None, None, :]).sum(axis=2), (values < floor).sum(axis=2), valid.all(axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-centres", type=int, default=16)
    ap.add_argument("--workloads", default="analysis_128,bench_256")
    ap.add_argument("--rotations", type=int, default=4096)
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    ctx = _native.default_context()
    rot = ccp4.rotationLattice(args.rotations)
    for name in args.workloads.split(","):
        if name == "analysis_128":
            spec, header, st, params, dens, diff, rot_mats = synthetic.cube_entry((128, 128, 128), 400, 5, 0.5)
            grid, n_centres, (frag, w) = np.asarray(diff, dtype=np.float32), 500, fragment(20, 4.0, 5)
        else:
            spec = synthetic.MapSpec(ncrs=(256, 256, 256), spacing=0.5)
            grid, n_centres, (frag, w) = synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5), 2000, fragment(40, 5.0, 6)
        dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "synth", ctx=ctx)
        nc, nr, ns = (int(v) for v in dm.header.ncrs)
        rng = np.random.default_rng(12)
        crs = np.stack([rng.integers(nc // 4, 3 * nc // 4, n_centres), rng.integers(nr // 4, 3 * nr // 4, n_centres), rng.integers(ns // 4, 3 * ns // 4, n_centres)], axis=1)
        centres = np.asarray(dm.header.crs2xyz_array(crs), dtype=np.float64) + rng.uniform(-0.25, 0.25, size=(n_centres, 3))
        floor = float(np.float32(0.0))
        rule = dict(top_k=5, floor=floor, max_low=len(frag) // 2)
        times = {"pose_scores": [], "pose_scores_global_only": [], "host_route_slice": [], "map_upload": []}
        got = None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            got = dm._map.pose_scores(frag, w, rot, centres, **rule)
            t1 = time.perf_counter()
            direct = dm._map.pose_scores(frag, w, rot, centres, global_only=True, **rule)
            t2 = time.perf_counter()
            if rep >= args.warmup:
                times["pose_scores"].append(t1 - t0)
                times["pose_scores_global_only"].append(t2 - t1)
        same = all(got[k].tobytes() == direct[k].tobytes() for k in ("bestRot", "bestScore", "bestLow", "nKept"))
        part = centres[:args.route_centres]
        for rep in range(1 + 3):
            ctx.synchronize()
            t0 = time.perf_counter()
            route = host_route(dm, frag, w, rot, part, floor)
            if rep >= 1:
                times["host_route_slice"].append(time.perf_counter() - t0)
        table = dm._map.pose_scores(frag, w, rot, part, full=True, **rule)
        worst = float(np.abs(table["scores"] - route[0]).max())
        for rep in range(1 + 3):
            ctx.synchronize()
            t0 = time.perf_counter()
            _native.DeviceMap(ctx, grid, dm.header.geometry())
            ctx.synchronize()
            if rep >= 1:
                times["map_upload"].append(time.perf_counter() - t0)
        ctx.profile_begin()
        dm._map.pose_scores(frag, w, rot, centres, **rule)
        staged_ms = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        ctx.profile_begin()
        dm._map.pose_scores(frag, w, rot, centres, global_only=True, **rule)
        global_ms = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        poses = n_centres * len(rot)
        slice_poses = len(part) * len(rot)
        out = {"workload": name, "grid": [nc, nr, ns], "centres": n_centres, "rotations": len(rot), "atoms": len(frag), "poses": poses, "samples": poses * len(frag),
               "reps": args.reps, "median_ms": med, "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v},
               "kernel_ms_staged": staged_ms, "kernel_ms_global_only": global_ms, "counters": got["counters"], "counters_global_only": direct["counters"],
               "paths_agree_to_the_byte": same,
               "ns_per_pose": {"pose_scores": round(1e6 * med["pose_scores"] / poses, 3), "host_route": round(1e6 * med["host_route_slice"] / slice_poses, 3)},
               "host_route_slice_centres": len(part),
               "host_route_whole_workload_ms_ESTIMATE_from_the_slice": round(med["host_route_slice"] * n_centres / len(part), 1),
               "host_route_bytes_up_down_whole_workload": [24 * poses * len(frag), 9 * poses * len(frag)],
               "host_route_max_abs_score_difference_on_the_slice": worst,
               "map_upload_GB_per_s": round(grid.nbytes / (1e6 * med["map_upload"]), 2)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
