"""The atom gradient sums (pdbeda_atom_moments), the adjoint of the model density, against the host route a user would write without them:
for every atom the box of voxels around it, the distances, the sphere test, numpy's exp and five weighted sums.  The two workloads of
tools/time_model.py:

  analysis_128  bench.py's analysis entry: 128^3, 2 000 atoms times their symmetry images, the single-Gaussian model of
                ccp4.gaussianAtomTerms with the defaults (cut-off 4 sigma); the weight map is the residual 2Fo-Fc - s model - o;
  bench_256     a 256^3 map (the size of bench.py's flagship map) with 50 000 atoms at bond-length spacing, B = 15 .. 40; the weight map
                is the noise map itself.

One `DensityMatrix.atomMoments` call per repetition; medians after warm-up; the kernel by HIP events in a call of its own; the counters of
the call.  The forward call (`modelDensity`) of the same atoms is timed beside it.  The host route is timed on at most --host-atoms atoms
and reported per atom beside the device's; the device's sums of the same atoms are compared with it.  One whole refinement cycle
(`refineGaussianAtoms(cycles=1)`: model, fit, residual, gradient sums, step, the trial model and its fit) is timed on the atoms of the
workload, every atom its own asymmetric unit.  --only-device leaves the host route out (a profiler run of the new kernel).  The figures are
written into DESIGN.md 4.18."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_model import walk      # noqa: E402


def host_route(header, weight, xyz, expo, radii):
    """The same sums on the host (orthogonal maps that start at 0: the tool's own): a box loop over the atoms.  (n, 5) for one term."""
    nc, nr, ns = (int(v) for v in header.ncrs)
    origin, length = np.asarray(header.origin, dtype=np.float64), np.asarray(header.gridLength, dtype=np.float64)
    axis = [np.arange(n) * length[header.map2crs[k]] + origin[header.map2crs[k]] for k, n in enumerate((nc, nr, ns))]          # coordinate along c, r, s
    out = np.zeros((len(xyz), 5))
    for i, (p, e, r) in enumerate(zip(xyz, expo[:, 0], radii.astype(np.float64))):
        lo, hi = [], []
        for k, n in enumerate((nc, nr, ns)):
            x = header.map2crs[k]
            lo.append(max(int(np.floor((p[x] - r - origin[x]) / length[x])), 0))
            hi.append(min(int(np.ceil((p[x] + r - origin[x]) / length[x])) + 1, n))
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        d = [axis[k][lo[k]:hi[k]] - p[header.map2crs[k]] for k in range(3)]
        dc, dr, ds = np.broadcast_arrays(d[0][None, None, :], d[1][None, :, None], d[2][:, None, None])
        d2 = (dc ** 2 + dr ** 2) + ds ** 2
        t0 = np.where(np.sqrt(d2) <= r, weight[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] * np.exp(-(e * d2)), 0.0)
        along = {header.map2crs[0]: dc, header.map2crs[1]: dr, header.map2crs[2]: ds}          # offsets along x, y, z
        out[i] = [t0.sum(), (t0 * along[0]).sum(), (t0 * along[1]).sum(), (t0 * along[2]).sum(), (t0 * d2).sum()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-atoms", type=int, default=5000)
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
            fit = an.modelCorrelation()
            weight = dm._residual(an.modelDensityObj, fit["scale"], fit["offset"])
            atoms = an._refinementAtoms()
            z, b, occ = atoms["electrons"][atoms["rows"]], atoms["bfactors"][atoms["rows"]], atoms["occupancies"][atoms["rows"]]
        else:
            spec = synthetic.MapSpec(ncrs=(256, 256, 256), spacing=0.5)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5))), "synth", ctx=ctx)
            xyz = walk(50000, np.zeros(3), np.full(3, 127.5), seed=21)
            z, b, occ = np.full(len(xyz), 7.0), np.random.default_rng(4).uniform(15.0, 40.0, len(xyz)), np.ones(len(xyz))
            amp, expo, b_eff = ccp4.gaussianAtomTerms(z, b, occ)
            radii = ccp4.modelRadii(b_eff)
            weight = dm
        amp, expo = np.ascontiguousarray(amp).reshape(len(xyz), -1), np.ascontiguousarray(expo).reshape(len(xyz), -1)
        header = dm.header
        times = {"atom_moments": [], "atom_moments_unique_box": [], "model_density": [], "refine_cycle": [], "host_route": []}
        got = None
        weight.atomMoments(xyz[:1], expo[:1], radii[:1])          # (the map's range pass, once: cached with the map)
        for rep in range(args.warmup + args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            got = weight.atomMoments(xyz, expo, radii)
            t1 = time.perf_counter()
            weight.atomMoments(xyz, expo, radii, uniqueBox=True)
            t2 = time.perf_counter()
            dm.modelDensity(xyz, amp, expo, radii)
            t3 = time.perf_counter()
            if rep >= args.warmup:
                times["atom_moments"].append(t1 - t0)
                times["atom_moments_unique_box"].append(t2 - t1)
                times["model_density"].append(t3 - t2)
        for rep in range(1 + 3):
            ctx.synchronize()
            t0 = time.perf_counter()
            cycle = dm.refineGaussianAtoms(xyz, z, b, occ, what=("xyz", "b"), cycles=1)
            if rep >= 1:
                times["refine_cycle"].append(time.perf_counter() - t0)
        host_n, worst, top = 0, None, None
        if not args.only_device:
            pick = np.arange(len(xyz)) if len(xyz) <= args.host_atoms else np.sort(np.random.default_rng(1).choice(len(xyz), args.host_atoms, replace=False))
            host_n = len(pick)
            grid = weight.density.astype(np.float64)
            t0 = time.perf_counter()
            want = host_route(header, grid, xyz[pick], expo[pick], radii[pick])
            times["host_route"].append(time.perf_counter() - t0)
            mine = got["moments"][pick, 0, :]
            worst, top = float(np.abs(mine - want).max()), float(np.abs(want).max())
        ctx.profile_begin()
        weight.atomMoments(xyz, expo, radii)
        dm.modelDensity(xyz, amp, expo, radii)
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        pairs = int(got["nVoxels"].astype(np.int64).sum())
        boxes = float(np.sum((2.0 * radii.astype(np.float64) / 0.5 + 1.0) ** 3))
        out = {"workload": name, "grid": [int(v) for v in header.ncrs], "atoms": len(xyz), "mean_radius": round(float(radii.mean()), 3), "reps": args.reps, "median_ms": med,
               "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "kernel_ms": prof, "counters": got["counters"],
               "pairs": pairs, "ns_per_pair": round(1e6 * prof.get("k_atom_moments", float("nan")) / max(pairs, 1), 4),
               "box_voxels_estimate": int(boxes), "refine_cycle_trace_T": cycle["trace"]["T"], "refine_cycle_halvings": cycle["trace"]["halvings"],
               "host_route_atoms": host_n, "host_max_abs_difference": worst, "host_max_abs_sum": top,
               "us_per_atom": {"atom_moments": round(1e3 * med["atom_moments"] / len(xyz), 3), "model_density": round(1e3 * med["model_density"] / len(xyz), 3),
                               "host_route": round(1e3 * med["host_route"] / host_n, 3) if host_n else None}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
