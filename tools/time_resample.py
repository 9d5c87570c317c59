"""Map resampling under coordinate operators (pdbeda_map_resample) against the host route a user would write without it: download
``density``, scipy.ndimage.map_coordinates(mode="grid-wrap") per operator in fp64, upload the result as a new map.  Workloads, on periodic
maps of smoothed noise at 0.4 A:

  rot128-o1 / -o3     a 128^3 map onto its own grid under a general rotation plus shift, trilinear and tricubic;
  rot256-o1 / -o3     the same at 256^3 (the flagship map's size);
  fine64-o3           a 64^3 box at a quarter of the spacing out of the 256^3 map, tricubic (a ligand's surroundings at 0.1 A);
  expand4-o1          the whole 128^3 cell from a 68 x 68 x 128 cut-out of it under four operators (the identity and three two-folds), first valid.

One call per repetition; medians of --reps after --warmup runs; the kernel by HIP events; each with staged boxes and with direct loads only
(PDBEDA_RESAMPLE_STAGE=0), the two results compared to the bit.  Each device time is also stated as a multiple of the time its MINIMAL
traffic would take at the device-to-device copy rate measured in the same run (a 256 MiB torch copy): 4 bytes read and 4 written per
destination voxel and operator.  --only-device leaves the host route out.  The figures are written into DESIGN.md 4.15."""
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

STAGE_SWITCH = "PDBEDA_RESAMPLE_STAGE"


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


def rigid(rotvec, about, shift):
    v = np.asarray(rotvec, dtype=np.float64)
    angle = float(np.linalg.norm(v))
    k = v / angle
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    rot = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * K.dot(K)
    about = np.asarray(about, dtype=np.float64)
    return np.hstack([rot, (about - rot.dot(about) + np.asarray(shift, dtype=np.float64)).reshape(3, 1)])


def host_route(dm, header, ops, order, ctx):
    """download + map_coordinates per operator (all of them evaluated: a host user has no early exit worth writing) + upload; seconds."""
    from scipy import ndimage
    from pdb_eda_amd import ccp4
    t0 = time.perf_counter()
    host = dm._map.download().astype(np.float64)
    src = dm.header
    if list(src.ncrs) != list(src.crsInterval):          # a cut-out that starts at 0: the rest of its cell is NaN
        cell = np.full((src.crsInterval[2], src.crsInterval[1], src.crsInterval[0]), np.nan)
        cell[:src.ncrs[2], :src.ncrs[1], :src.ncrs[0]] = host
        host = cell
    nc, nr, ns = (int(v) for v in header.ncrs)
    s, r, c = np.meshgrid(np.arange(ns), np.arange(nr), np.arange(nc), indexing="ij")
    xyz = header.crs2xyz_array(np.stack([c.ravel(), r.ravel(), s.ravel()], axis=1))
    out = None
    for op in ops:
        moved = xyz.dot(op[:, :3].T) + op[:, 3]
        f = (moved - np.asarray(src.origin)) / np.asarray(src.gridLength)          # (orthogonal maps, x = c)
        value = ndimage.map_coordinates(host, [f[:, 2], f[:, 1], f[:, 0]], order=order, mode="grid-wrap")
        out = value if out is None else np.where(np.isnan(out), value, out)        # the first operator that finds density
    out = np.nan_to_num(out)
    ccp4.DensityMatrix(header, header.origin, out.astype(np.float32).reshape(ns, nr, nc), "host", ctx=ctx)
    ctx.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    copy_gbs = copy_rate_gbs()
    ctx = _native.default_context()
    maps = {}

    def periodic(n):
        if n not in maps:
            spec = synthetic.MapSpec(ncrs=(n, n, n), spacing=0.4)
            maps[n] = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5))), "synth", ctx=ctx)
        return maps[n]

    def workloads():
        for n in (128, 256):
            dm = periodic(n)
            centre = np.full(3, 0.2 * n)
            for order in (1, 3):
                yield "rot%d-o%d" % (n, order), dm, dm.header, [rigid((0.2, -0.3, 0.4), centre, (0.31, -0.17, 0.23))], order
        dm = periodic(256)
        yield "fine64-o3", dm, ccp4.boxHeader(np.full(3, 51.2), 3.1, 0.1), [rigid((0.2, -0.3, 0.4), np.full(3, 51.2), (0.03, 0.02, -0.01))], 3
        spec = synthetic.MapSpec(ncrs=(68, 68, 128), interval=(128, 128, 128), spacing=0.4)          # a little more than a quarter of a P222-like cell
        dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=11, sigma_voxels=1.5))), "synth", ctx=ctx)
        folds = [np.hstack([np.diag(d), np.zeros((3, 1))]) for d in ([1.0, 1.0, 1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, -1.0])]
        yield "expand4-o1", dm, ccp4.cellHeader(dm.header), folds, 1

    only = set(v for v in args.only.split(",") if v)
    for name, dm, header, ops, order in workloads():
        if only and name not in only:
            continue
        ops = np.array(ops, dtype=np.float64).reshape(-1, 3, 4)
        flat = ops.reshape(-1, 12)
        times, results, counters, kernel = {}, {}, {}, {}
        for label, switch in (("staged", "1"), ("direct", "0")):
            os.environ[STAGE_SWITCH] = switch
            runs = []
            for rep in range(args.warmup + args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = dm.resampled(header, flat, order=order)
                t1 = time.perf_counter()
                if rep >= args.warmup:
                    runs.append(t1 - t0)
            times[label] = runs
            results[label] = out.density
            counters[label] = out.resampleCounters
            ctx.profile_begin()
            dm.resampled(header, flat, order=order)
            kernel[label] = round(ctx.profile_end()["k_map_resample"][1], 4)
        del os.environ[STAGE_SWITCH]
        voxels = int(header.ncrs[0]) * int(header.ncrs[1]) * int(header.ncrs[2])
        floor_ms = 8.0 * voxels * len(ops) / (copy_gbs * 1e9) * 1e3
        host = None
        if not args.only_device:
            host = [host_route(dm, header, ops, order, ctx) for _ in range(2)]
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items()}
        out = {"workload": name, "source": [int(v) for v in dm.header.ncrs], "destination": [int(v) for v in header.ncrs], "operators": len(ops), "order": order, "reps": args.reps,
               "median_ms": med, "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items()}, "kernel_ms": kernel, "counters": counters,
               "staged_equals_direct": bool(results["staged"].tobytes() == results["direct"].tobytes()), "copy_rate_GBs": round(copy_gbs, 1),
               "min_traffic_ms": round(floor_ms, 4), "call_over_min_traffic": {k: round(v / floor_ms, 2) for k, v in med.items()},
               "kernel_over_min_traffic": {k: round(v / floor_ms, 2) for k, v in kernel.items()},
               "staged_over_direct_kernel": round(kernel["staged"] / kernel["direct"], 3),
               "host_route_ms": round(1e3 * statistics.median(host), 1) if host else None,
               "host_route_over_device": round(statistics.median(host) * 1e3 / med["staged"], 1) if host else None}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
