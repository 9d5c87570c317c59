"""The calculated density of a model (pdbeda_model_density) and the map-model sums (pdbeda_map_pair_moments) against the host route a
user would write without them: for every atom the box of voxels around it, the distances, the sphere test and numpy's exp, added into a
float64 grid.  Two workloads:

  analysis_128  bench.py's analysis entry: 128^3, 2 000 atoms times their symmetry images, the single-Gaussian model of
                ccp4.gaussianAtomTerms with the defaults (cut-off 4 sigma);
  bench_256     a 256^3 map (the size of bench.py's flagship map) with 50 000 atoms at bond-length spacing, B = 15 .. 40.

One `DensityMatrix.modelDensity` call per repetition; medians after warm-up; the kernels by HIP events; the staging counters of the call.
The host route is timed on at most --host-atoms atoms and reported per atom beside the device's; the device's map of the same atoms is
compared with it.  The 256^3 workload also times `pairMoments` of the observed map against the calculated one, beside the time it takes
to stream the 8 bytes per voxel once at --hbm-gbs.  --only-device leaves the host route out (a profiler run of the new kernels).  The
figures are written into DESIGN.md 4.12."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def walk(n, lo, hi, seed, bond=1.5):
    """``n`` atoms: a random walk of ``bond``-long steps folded back into the box [lo, hi] (tools/time_qscore.py's)."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n, 3))
    steps *= bond / np.linalg.norm(steps, axis=1)[:, None]
    steps[0] = rng.uniform(0.0, hi - lo)
    span = hi - lo
    pos = np.mod(np.cumsum(steps, axis=0), 2.0 * span)
    return lo + np.where(pos > span, 2.0 * span - pos, pos)


def host_route(header, xyz, amp, expo, radii):
    """The same map on the host (orthogonal maps that start at 0: the tool's own): a box loop over the atoms."""
    nc, nr, ns = (int(v) for v in header.ncrs)
    grid = np.zeros((ns, nr, nc))
    origin, length = np.asarray(header.origin, dtype=np.float64), np.asarray(header.gridLength, dtype=np.float64)
    axis = [np.arange(n) * length[header.map2crs[k]] + origin[header.map2crs[k]] for k, n in enumerate((nc, nr, ns))]          # coordinate along c, r, s
    for p, a, e, r in zip(xyz, amp, expo, radii.astype(np.float64)):
        lo, hi = [], []
        for k, n in enumerate((nc, nr, ns)):
            x = header.map2crs[k]
            lo.append(max(int(np.floor((p[x] - r - origin[x]) / length[x])), 0))
            hi.append(min(int(np.ceil((p[x] + r - origin[x]) / length[x])) + 1, n))
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        d = [axis[k][lo[k]:hi[k]] - p[header.map2crs[k]] for k in range(3)]
        d2 = (d[0][None, None, :] ** 2 + d[1][None, :, None] ** 2) + d[2][:, None, None] ** 2
        inside = np.sqrt(d2) <= r
        grid[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] += np.where(inside, (a[None, None, None, :] * np.exp(-(e[None, None, None, :] * d2[..., None]))).sum(axis=3), 0.0)
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-atoms", type=int, default=5000)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the streaming floor is quoted against, GB/s")
    ap.add_argument("--workloads", default="analysis_128,bench_256")
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic, structure, densityAnalysis as da
    ctx = _native.default_context()
    for name in args.workloads.split(","):
        if name == "analysis_128":
            spec, header, st, params, dens, diff, rot = synthetic.cube_entry((128, 128, 128), 400, 5, 0.5)
            da.setGlobals(params)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), "synth", ctx=ctx)
            diffObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), "synth", ctx=ctx)
            da._attachCutoffs(dm, diffObj)
            an = da.DensityAnalysis("synth", dm, diffObj, st, structure.PDBEntry(structure.PDBHeader(pdbid="synth", resolution=2.0, spaceGroup="P_1", rotationMats=rot)))
            xyz, amp, expo, radii, _ = an._modelAtoms()
        else:
            spec = synthetic.MapSpec(ncrs=(256, 256, 256), spacing=0.5)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5))), "synth", ctx=ctx)
            xyz = walk(50000, np.zeros(3), np.full(3, 127.5), seed=21)
            amp, expo, b_eff = ccp4.gaussianAtomTerms(np.full(len(xyz), 7.0), np.random.default_rng(4).uniform(15.0, 40.0, len(xyz)), np.ones(len(xyz)))
            radii = ccp4.modelRadii(b_eff)
        amp, expo = np.ascontiguousarray(amp).reshape(len(xyz), -1), np.ascontiguousarray(expo).reshape(len(xyz), -1)
        header = dm.header
        times = {"model_density": [], "pair_moments": [], "host_route": []}
        model = None
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            model = dm.modelDensity(xyz, amp, expo, radii)
            t1 = time.perf_counter()
            dm.pairMoments(model)
            t2 = time.perf_counter()
            if rep >= args.warmup:
                times["model_density"].append(t1 - t0)
                times["pair_moments"].append(t2 - t1)
        counters = model.modelCounters
        host_n, worst, top = 0, None, None
        if not args.only_device:
            pick = np.arange(len(xyz)) if len(xyz) <= args.host_atoms else np.sort(np.random.default_rng(1).choice(len(xyz), args.host_atoms, replace=False))
            host_n = len(pick)
            t0 = time.perf_counter()
            want = host_route(header, xyz[pick], amp[pick], expo[pick], radii[pick])
            times["host_route"].append(time.perf_counter() - t0)
            got = dm.modelDensity(xyz[pick], amp[pick], expo[pick], radii[pick]).density
            worst, top = float(np.abs(got - want).max()), float(want.max())
        ctx.profile_begin()
        dm.pairMoments(dm.modelDensity(xyz, amp, expo, radii))
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        voxels = int(np.prod(header.ncrs))
        pairs = float(np.sum(4.0 / 3.0 * np.pi * radii.astype(np.float64) ** 3) / header.unitVolume)          # (voxel, atom) pairs inside a sphere
        fit = dm.correlate(model)
        out = {"workload": name, "grid": [int(v) for v in header.ncrs], "atoms": len(xyz), "mean_radius": round(float(radii.mean()), 3), "reps": args.reps, "median_ms": med,
               "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "kernel_ms": prof, "counters": counters,
               "pairs_inside_spheres": int(pairs), "ns_per_pair_inside": round(1e6 * prof.get("k_model_tile", float("nan")) / pairs, 4),
               "pair_moments_floor_ms_at_%g_GBs" % args.hbm_gbs: round(8.0 * voxels / (args.hbm_gbs * 1e9) * 1e3, 4),
               "pair_moments_kernel_GBs": round(8.0 * voxels / (prof.get("k_pair_moments", float("nan")) * 1e-3) / 1e9, 1), "cc_with_the_observed_map": round(fit["cc"], 4),
               "host_route_atoms": host_n, "host_max_abs_difference": worst, "host_max_voxel": top,
               "us_per_atom": {"model_density": round(1e3 * med["model_density"] / len(xyz), 3), "host_route": round(1e3 * med["host_route"] / host_n, 3) if host_n else None}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
