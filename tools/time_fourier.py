"""Reciprocal space (pdbeda_map_fft, pdbeda_spectrum_inverse, pdbeda_spectrum_scale, pdbeda_spectrum_shells and ``DensityMatrix.resolutionCut``
on top of them) against the host route a user would write without them: download ``density``, numpy.fft.rfftn / irfftn in fp64, upload the
result as a new map.  Two periodic maps, 128^3 and 256^3 (the sizes of bench.py's analysis entry and flagship map):

  forward          ``DensityMatrix.fourier``;
  inverse          ``DensitySpectrum.toMap``;
  scale            ``DensitySpectrum.scale`` with a 1024-entry table;
  shells_pair      ``DensitySpectrum.shells`` of two spectra, 20 shells;
  resolution_cut   ``DensityMatrix.resolutionCut`` at 3 A: transform, scale, inverse transform.

One call per repetition; medians after warm-up; the kernels by HIP events, one profiled call each.  Each device time is also stated as a
multiple of the time its MINIMAL traffic would take at the device-to-device copy rate measured in the same run (a 256 MiB torch copy).  Per
voxel a transform moves 44 bytes -- 4 in and 8 out in the pass along c (the half spectrum is 8 bytes a voxel), 8 in and 8 out in each of the
passes along r and s --, the scale 16, the shells of a pair 16, the resolution cut 44 + 16 + 44.  ``passes`` states every transform kernel
against ITS share of that traffic, which shows the pass that is furthest from its floor.  --only-device leaves the host route out.  The
result goes to --out (one JSON object per size, a list) and to stdout; the figures are quoted in README.md and DESIGN.md 4.16."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"forward": 44, "inverse": 44, "scale": 16, "shells_pair": 16, "resolution_cut": 104}
PASS_BYTES = {"k_fft_rows": 12, "k_fft_cols_r": 16, "k_fft_cols_s": 16, "k_ifft_rows": 12}


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


def profiled(ctx, call):
    ctx.profile_begin()
    call()
    return {k: (cnt, round(ms, 4)) for k, (cnt, ms) in sorted(ctx.profile_end().items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--cut", type=float, default=3.0, help="Angstrom")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_fourier_time.json"))
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic
    copy_gbs = copy_rate_gbs()
    ctx = _native.default_context()
    results = []
    for n in (int(v) for v in args.sizes.split(",")):
        spec = synthetic.MapSpec(ncrs=(n, n, n), spacing=0.4)
        ga = synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5)
        gb = synthetic.noise_grid(spec, seed=10, sigma_voxels=1.5)
        a = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, ga)), "synth", ctx=ctx)
        b = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, gb)), "synth", ctx=ctx)
        edges = ccp4.shellEdges(a.header, 20)
        s2max = ccp4.maxS2(a.header)
        table = ccp4.bFactorTable(0.0, s2max)          # (all ones: repeated scaling leaves the spectrum as it is)
        spec_b = b.fourier()
        times = dict((k, []) for k in list(BYTES) + ["host_route", "host_rfftn", "host_irfftn", "host_download", "host_upload"])
        cut = None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            spec_a = a.fourier()
            t1 = time.perf_counter()
            spec_a.toMap()
            t2 = time.perf_counter()
            spec_a.scale(table, s2max, 0.0)
            t3 = time.perf_counter()
            spec_a.shells(spec_b, edges=edges)
            t4 = time.perf_counter()
            cut = a.resolutionCut(args.cut)
            t5 = time.perf_counter()
            if rep >= args.warmup:
                for key, dt in zip(BYTES, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    times[key].append(dt)
        worst = None
        if not args.only_device:
            soft = 0.1
            g = None
            for rep in range(2):
                t0 = time.perf_counter()
                host = a._map.download()
                t1 = time.perf_counter()
                f = np.fft.rfftn(host.astype(np.float64))
                t2 = time.perf_counter()
                if g is None:      # (the radial window is not part of the route's time: the device call gets its table from the host too)
                    m = ccp4.reciprocalMetric(a.header)
                    h = [np.where(2 * np.arange(n) <= n, np.arange(n), np.arange(n) - n).astype(np.float64) for _ in range(3)]
                    s2 = m[0] * h[0][None, None, :n // 2 + 1] ** 2 + m[1] * h[1][None, :, None] ** 2 + m[2] * h[2][:, None, None] ** 2
                    g = np.interp(s2, np.linspace(0.0, ((1.0 + 0.5 * soft) / args.cut) ** 2 * (1.0 + 2.0 ** -20), 1024), ccp4.resolutionTable(args.cut, None, soft), right=0.0)
                    t2 = time.perf_counter()
                back = np.fft.irfftn(f * g, s=host.shape, axes=(0, 1, 2))
                t3 = time.perf_counter()
                ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, back.astype(np.float32))), "synth", ctx=ctx)
                ctx.synchronize()
                t4 = time.perf_counter()
                if rep == 1:
                    for key, dt in (("host_route", t4 - t0), ("host_download", t1 - t0), ("host_rfftn", t2 - t1), ("host_irfftn", t3 - t2), ("host_upload", t4 - t3)):
                        times[key].append(dt)
            worst = float(np.abs(cut.density.astype(np.float64) - back).max())
        prof = {"forward": profiled(ctx, lambda: a.fourier())}
        keep = a.fourier()
        prof["inverse"] = profiled(ctx, lambda: keep.toMap())
        prof["scale"] = profiled(ctx, lambda: keep.scale(table, s2max, 0.0))
        prof["shells_pair"] = profiled(ctx, lambda: keep.shells(spec_b, edges=edges))
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        voxels = n ** 3
        floor = {k: BYTES[k] * voxels / (copy_gbs * 1e9) * 1e3 for k in BYTES}
        kernels = {k: round(sum(ms for _, ms in prof[k].values()), 4) for k in prof}
        passes = {}
        for which in ("forward", "inverse"):
            for name, (cnt, ms) in prof[which].items():
                share = PASS_BYTES.get(name)
                if share:
                    passes["%s/%s" % (which, name)] = {"ms": ms, "over_min_traffic": round(ms / (share * voxels / (copy_gbs * 1e9) * 1e3), 2)}
        out = {"grid": [n, n, n], "reps": args.reps, "median_ms": med, "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v},
               "kernels_count_ms": prof, "kernels_ms": kernels, "copy_rate_GBs": round(copy_gbs, 1),
               "min_traffic_ms": {k: round(v, 4) for k, v in floor.items()},
               "call_over_min_traffic": {k: round(med[k] / floor[k], 2) for k in BYTES},
               "kernels_over_min_traffic": {k: round(kernels[k] / floor[k], 2) for k in kernels},
               "passes": passes,
               "host_route_over_resolution_cut": round(med["host_route"] / med["resolution_cut"], 1) if "host_route" in med else None,
               "max_abs_resolution_cut_minus_numpy": worst}
        results.append(out)
        print(json.dumps(out), flush=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
