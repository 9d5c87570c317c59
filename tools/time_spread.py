"""The ordered spread of a mask (pdbeda_map_spread) on an MI355X, in one process: 128^3 and 256^3 periodic maps at 0.4 A whose mask is
thresholded smooth noise with about 40 % of the voxels set.  Timed: `dilated` at 1 A and at 3 A, `distanceFrom` at 3 A, the rows path against
the ordered walk (PDBEDA_SPREAD_ROWS=0, read at every call) at 3 A, and `solventMask` on the 50 000-atom walk of tools/time_model.py (256^3 at
0.5 A).  Medians of --reps calls after --warmup; the kernels by HIP events (the context's profile) in a call of their own.

Each figure stands beside two others of the same run: the time of the minimal traffic -- 4 B read and 4 B written per voxel -- at the
device-to-device copy rate measured here, and the host route: download, scipy (binary_dilation at 1 A; distance_transform_edt at 3 A, which
is how a host would dilate by a large ball as well) on the wrap-padded array, upload.  One JSON line per workload."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, ctx, reps, warmup):
    times = []
    for rep in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if rep >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(times), 4)


def kernel_ms(fn, ctx):
    ctx.profile_begin()
    fn()
    return {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}


def copy_rate_gbs():
    """Read + written bytes per second of a device-to-device copy of 256 MiB (bench.py's ceiling; tools/time_fourier.py's), GB/s."""
    import torch
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


def host_route(dm, threshold, spacing, radius, how):
    """Download, scipy on the wrap-padded mask, upload: seconds -> ms, and the result for the comparison."""
    from scipy import ndimage
    from pdb_eda_amd import ccp4, synthetic
    t0 = time.perf_counter()
    x = np.array(dm._map.download())
    mask = x > np.float32(threshold)
    pad = int(np.floor(radius / spacing + 1e-9))
    wide = np.pad(mask, pad, mode="wrap")
    if how == "dilation":
        offsets = ccp4.spreadTable(dm.header, radius)[0]
        ball = np.zeros((2 * pad + 1,) * 3, dtype=bool)
        ball[offsets[:, 2] + pad, offsets[:, 1] + pad, offsets[:, 0] + pad] = True
        out = ndimage.binary_dilation(wide, structure=ball)[pad:-pad, pad:-pad, pad:-pad].astype(np.float32)
    else:
        edt = ndimage.distance_transform_edt(~wide, sampling=spacing)[pad:-pad, pad:-pad, pad:-pad]
        out = (edt <= radius + 1e-9).astype(np.float32) if how == "edt_dilation" else np.where(edt <= radius + 1e-9, edt, np.inf).astype(np.float32)
    type(dm._map)(dm._ctx, np.ascontiguousarray(out), dm.header.geometry())
    dm._ctx.synchronize()
    return round(1e3 * (time.perf_counter() - t0), 2), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="128,256,solvent")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    rate = copy_rate_gbs()          # (before the library's context, as the other tools do)
    ctx = _native.default_context()
    spacing = 0.4
    for name in args.workloads.split(","):
        if name == "solvent":
            sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
            import time_model
            spec = synthetic.MapSpec(ncrs=(256, 256, 256), spacing=0.5)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((256, 256, 256), dtype=np.float32))), "synth", ctx=ctx)
            xyz = time_model.walk(50000, np.zeros(3), np.full(3, 127.5), seed=21)
            radii = np.full(len(xyz), ccp4.MASK_VDW["C"])
            call = lambda: dm.solventMask(xyz, radii)
            out = {"workload": "solvent_mask_256", "grid": [256] * 3, "spacing": 0.5, "atoms": len(xyz), "probe": 1.11, "shrink": 0.9,
                   "median_ms": {"solventMask": median_ms(call, ctx, args.reps, args.warmup), "atomMask": median_ms(lambda: dm.atomMask(xyz, radii + 1.11), ctx, args.reps, args.warmup)},
                   "kernel_ms": kernel_ms(call, ctx), "solvent_fraction": float(np.asarray(call().density, dtype=np.float64).mean())}
            print(json.dumps(out), flush=True)
            continue
        n = int(name)
        spec = synthetic.MapSpec(ncrs=(n, n, n), spacing=spacing)
        grid = synthetic.noise_grid(spec, seed=9, sigma_voxels=3.0)
        threshold = float(np.quantile(grid, 0.6))
        dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "synth", ctx=ctx)
        n_bytes = 4 * n ** 3
        forms = {"dilated_1A": lambda: dm.dilated(1.0, threshold), "dilated_3A": lambda: dm.dilated(3.0, threshold), "distanceFrom_3A": lambda: dm.distanceFrom(3.0, threshold)}
        med = {k: median_ms(fn, ctx, args.reps, args.warmup) for k, fn in forms.items()}
        kern = {k: kernel_ms(fn, ctx) for k, fn in forms.items()}
        os.environ["PDBEDA_SPREAD_ROWS"] = "0"
        try:
            med["dilated_3A_walk"] = median_ms(forms["dilated_3A"], ctx, args.reps, args.warmup)
            med["distanceFrom_3A_walk"] = median_ms(forms["distanceFrom_3A"], ctx, args.reps, args.warmup)
            kern["dilated_3A_walk"] = kernel_ms(forms["dilated_3A"], ctx)
            kern["distanceFrom_3A_walk"] = kernel_ms(forms["distanceFrom_3A"], ctx)
            walked = np.array(forms["distanceFrom_3A"]().density)
        finally:
            del os.environ["PDBEDA_SPREAD_ROWS"]
        by_rows = np.array(forms["distanceFrom_3A"]().density)
        _, ctr = dm.spread(*_table(ccp4, dm, 3.0), threshold=threshold, counters=True)
        out = {"workload": "periodic_%d" % n, "grid": [n] * 3, "spacing": spacing, "mask_fraction": float((grid > np.float32(threshold)).mean()), "reps": args.reps,
               "offsets": {"1A": len(ccp4.spreadTable(dm.header, 1.0)[0]), "3A": len(ccp4.spreadTable(dm.header, 3.0)[0])}, "counters_3A": ctr,
               "median_ms": med, "kernel_ms": kern, "rows_equal_walk_bits": bool(np.array_equal(by_rows.view(np.uint32), walked.view(np.uint32))),
               "d2d_copy_gbs": round(rate, 1), "minimal_traffic_ms": round(2.0 * n_bytes / (1e6 * rate), 4)}          # (GB/s = 1e6 bytes per ms)
        if not args.no_host:
            host = {}
            host["dilated_1A"], want = host_route(dm, threshold, spacing, 1.0, "dilation")
            out["host_equal_dilated_1A"] = bool(np.array_equal(want, np.asarray(forms["dilated_1A"]().density)))
            host["dilated_3A"], want = host_route(dm, threshold, spacing, 3.0, "edt_dilation")
            out["host_equal_dilated_3A"] = bool(np.array_equal(want, np.asarray(forms["dilated_3A"]().density)))
            host["distanceFrom_3A"], want = host_route(dm, threshold, spacing, 3.0, "edt")
            with np.errstate(invalid="ignore"):          # (inf - inf where both say "beyond")
                out["host_max_abs_difference_distance_3A"] = float(np.nanmax(np.abs(np.where(np.isinf(want) & np.isinf(by_rows), 0.0, want - by_rows))))
            out["host_route_ms"] = host
        print(json.dumps(out), flush=True)


def _table(ccp4, dm, radius):
    offsets = ccp4.spreadTable(dm.header, radius)[0]
    return offsets, np.append(np.ones(len(offsets), dtype=np.float32), np.float32(0.0))


if __name__ == "__main__":
    main()
