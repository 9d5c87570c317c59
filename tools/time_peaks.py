"""Peak search: time of one call (enqueue + count + all columns, synchronised, after warm-up) of findPeakLists at 3 sigma and of
findPeaks at 1.5 sigma on a 256^3 synthetic map (smooth noise, the generator of the bench), with and without the blob lists
that give every peak its blob; the kernels (HIP events on the context's stream) and the host-side ordering of the list separately,
and the labelling kernel of the same map beside the stencil (both read the grid once).
    python tools/time_peaks.py [--edge 256] [--reps 20] [--out FILE]
Prints one JSON document.  Under `rocprofv3 --kernel-trace --stats -- python tools/time_peaks.py` the kernel times are the tool's."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, call, reps):
    """Median / min wall time of call() (which must end synchronised), and the per-kernel medians of one profiled repetition set."""
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
            "per_call_us": {name: round(1e3 * ms / reps, 2) for name, (calls, ms) in sorted(prof.items())}}


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
    dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "peaks", ctx=ctx)
    mean, std = dm.meanDensity, dm.stdDensity
    out = {"edge": a.edge, "voxels": a.edge ** 3, "grid_bytes": 4 * a.edge ** 3, "reps": a.reps, "rows": []}

    def whole(lists):
        for pl in lists:
            pl.rows()
            pl.free()

    cases = []
    c3, c15 = mean + 3 * std, mean + 1.5 * std
    cases.append(("findPeakLists 3 sigma", lambda: whole(dm._map.peaks_pm(c3, -c3))))
    cases.append(("findPeaks 1.5 sigma", lambda: whole([dm._map.peaks(c15)])))
    green, red = dm._map.full_blobs_pm(c3, -c3, labels=True)
    blue = dm._map.full_blobs(c15, labels=True)
    len(green), len(blue)
    cases.append(("findPeakLists 3 sigma + blobs", lambda: whole(dm._map.peaks_pm(c3, -c3, green, red))))
    cases.append(("findPeaks 1.5 sigma + blobs", lambda: whole([dm._map.peaks(c15, blue)])))

    def label(cut):
        bl = dm._map.full_blobs(cut)
        len(bl)
        bl.free()
    cases.append(("createFullBlobList 1.5 sigma (yardstick: k_tile_label)", lambda: label(c15)))
    for name, call in cases:
        row = {"case": name}
        row.update(timed(ctx, call, a.reps))
        if "Peak" in name:
            lists = dm._map.peaks_pm(c3, -c3) if "Lists" in name else [dm._map.peaks(c15)]
            row["peaks"] = [len(pl) for pl in lists]
            row["counters"] = [pl.counters() for pl in lists]
            stencil = row["per_call_us"].get("k_peak_stencil")
            if stencil:
                row["stencil_GBps"] = round(out["grid_bytes"] / (stencil * 1e-6) / 1e9, 1)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
