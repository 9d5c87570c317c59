"""The separable map filter (pdbeda_map_filter) and the local statistics (pdbeda_map_local_stats) against the host route a user would write
without them: download ``density``, scipy.ndimage.gaussian_filter(mode="wrap") in fp64, upload the result as a new map.  Two periodic maps,
128^3 and 256^3 (the sizes of bench.py's analysis entry and flagship map):

  gaussian_filter   ``DensityMatrix.gaussianFilter`` at sigma = 1.5 grid steps (radius 6);
  local_stats       ``DensityMatrix.localStats`` of a pair of maps at sigma = 7.5 grid steps cut off at 3 sigma (radius 23: the analysis
                    layer's 3 A window on a 0.4 A grid), all six outputs.

One call per repetition; medians after warm-up; the kernels by HIP events.  Each device time is also stated as a fraction of the time its
MINIMAL traffic would take at the device-to-device copy rate measured in the same run (a 256 MiB torch copy): the filter moves at least 40
bytes per voxel (4 read + 8 written, 8 + 8, 8 + 4), the local statistics of a pair 8 read + 40 written, 80 + 80 for the two other passes
of five channels, and 40 + 8 read + 24 written by the closing kernel: 280.  The host route of the local statistics is its five
gaussian_filter calls alone (no download or upload counted).  --only-device leaves the host route out.  The figures are written into
DESIGN.md 4.14."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch first)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILTER_BYTES_PER_VOXEL = 40
PAIR_STATS_BYTES_PER_VOXEL = 280


def copy_rate_gbs():
    """Read + written bytes per second of a device-to-device copy of 256 MiB (bench.py's ceiling)."""
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    return 10 * 2 * src.numel() * 4 / (a.elapsed_time(b) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--filter-sigma", type=float, default=1.5, help="grid steps")
    ap.add_argument("--stats-sigma", type=float, default=7.5, help="grid steps")
    ap.add_argument("--stats-truncate", type=float, default=3.0)
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    copy_gbs = copy_rate_gbs()
    ctx = _native.default_context()
    for n in (int(v) for v in args.sizes.split(",")):
        spec = synthetic.MapSpec(ncrs=(n, n, n), spacing=0.4)
        ga = synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5)
        gb = synthetic.noise_grid(spec, seed=10, sigma_voxels=1.5)
        a = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, ga)), "synth", ctx=ctx)
        b = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, gb)), "synth", ctx=ctx)
        times = {"gaussian_filter": [], "local_stats": [], "host_filter_route": [], "host_filter_scipy": [], "host_stats_scipy": []}
        out_f = out_s = None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            out_f = a.gaussianFilter(args.filter_sigma, voxels=True, renormalize=False)
            t1 = time.perf_counter()
            out_s = a.localStats(b, sigma=args.stats_sigma, truncate=args.stats_truncate, voxels=True)
            t2 = time.perf_counter()
            if rep >= args.warmup:
                times["gaussian_filter"].append(t1 - t0)
                times["local_stats"].append(t2 - t1)
        worst = worst_mean = None
        if not args.only_device:
            from scipy import ndimage
            for rep in range(2):
                t0 = time.perf_counter()
                host = a._map.download()
                t1 = time.perf_counter()
                smooth = ndimage.gaussian_filter(host.astype(np.float64), args.filter_sigma, mode="wrap")
                t2 = time.perf_counter()
                ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, smooth.astype(np.float32))), "synth", ctx=ctx)
                ctx.synchronize()
                t3 = time.perf_counter()
                times["host_filter_route"].append(t3 - t0)
                times["host_filter_scipy"].append(t2 - t1)
            worst = float(np.abs(out_f.density.astype(np.float64) - smooth).max())
            a64, b64 = ga.astype(np.float64), gb.astype(np.float64)
            t0 = time.perf_counter()
            moments = [ndimage.gaussian_filter(x, args.stats_sigma, mode="wrap", truncate=args.stats_truncate) for x in (a64, a64 * a64, b64, b64 * b64, a64 * b64)]
            times["host_stats_scipy"].append(time.perf_counter() - t0)
            worst_mean = float(np.abs(out_s["mean"].density.astype(np.float64) - moments[0]).max())
        ctx.profile_begin()
        a.gaussianFilter(args.filter_sigma, voxels=True, renormalize=False)
        prof_f = {k: (cnt, round(ms, 4)) for k, (cnt, ms) in sorted(ctx.profile_end().items())}
        ctx.profile_begin()
        a.localStats(b, sigma=args.stats_sigma, truncate=args.stats_truncate, voxels=True)
        prof_s = {k: (cnt, round(ms, 4)) for k, (cnt, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        voxels = n ** 3
        floor_f = FILTER_BYTES_PER_VOXEL * voxels / (copy_gbs * 1e9) * 1e3
        floor_s = PAIR_STATS_BYTES_PER_VOXEL * voxels / (copy_gbs * 1e9) * 1e3
        kern_f, kern_s = sum(ms for _, ms in prof_f.values()), sum(ms for _, ms in prof_s.values())
        out = {"grid": [n, n, n], "reps": args.reps, "filter_radius": len(ccp4.gaussianTaps(args.filter_sigma)) // 2,
               "stats_radius": len(ccp4.gaussianTaps(args.stats_sigma, args.stats_truncate)) // 2, "median_ms": med,
               "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "filter_kernels_count_ms": prof_f, "stats_kernels_count_ms": prof_s,
               "copy_rate_GBs": round(copy_gbs, 1), "filter_min_traffic_ms": round(floor_f, 4), "stats_min_traffic_ms": round(floor_s, 4),
               "filter_call_over_min_traffic": round(med["gaussian_filter"] / floor_f, 2), "filter_kernels_over_min_traffic": round(kern_f / floor_f, 2),
               "stats_call_over_min_traffic": round(med["local_stats"] / floor_s, 2), "stats_kernels_over_min_traffic": round(kern_s / floor_s, 2),
               "host_route_over_device_filter": round(med["host_filter_route"] / med["gaussian_filter"], 1) if "host_filter_route" in med else None,
               "host_scipy_over_device_stats": round(med["host_stats_scipy"] / med["local_stats"], 1) if "host_stats_scipy" in med else None,
               "max_abs_filter_minus_scipy": worst, "max_abs_local_mean_minus_scipy": worst_mean}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
