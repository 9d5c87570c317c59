"""Radial profiles against what the library offered before them, on the 128^3 / 2 000-atom analysis entry of bench.py:

  one call     DensityAnalysis.calculateAtomRadialProfiles(2.0, 20): ONE launch (k_atom_shells), rows included;
  the device   DeviceMap.radial_profiles alone (no table rows), and its HIP-event kernel time;
  twenty calls the same curve from pdbeda_region_sums: one call per radius k * w, k = 1..20, differenced.

Medians over --reps repetitions after warm-up, all in this process, interleaved (a repetition runs every form once).  The
figures are written into DESIGN.md 4.6 (the table's time is the 160 000 Python numbers of its list columns: see there)."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", default="c2_bench_entry")
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native, ccp4, synthetic, structure, densityAnalysis as da
    ctx = _native.default_context()
    ncrs, n_res, seed, spacing = synthetic.BIG_CASES[args.case]
    spec, header, st, params, dens, diff, rot = synthetic.cube_entry(ncrs, n_res, seed, spacing)
    da.setGlobals(params)
    densityObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), "synth", ctx=ctx)
    diffObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), "synth", ctx=ctx)
    da._attachCutoffs(densityObj, diffObj)
    an = da.DensityAnalysis("synth", densityObj, diffObj, st, structure.PDBEntry(structure.PDBHeader(pdbid="synth", resolution=2.0, spaceGroup="P_1", rotationMats=rot)))
    xyz = structure.columns(st).coord
    n_atoms, radius, shells = len(xyz), 2.0, 20
    cut = densityObj.meanDensity + 1.5 * densityObj.stdDensity
    off = np.arange(n_atoms + 1, dtype=np.int64)
    width = float(np.float32(radius)) / shells
    radii = [np.full(n_atoms, np.float32((k + 1) * width), dtype=np.float32) for k in range(shells)]
    radii[-1][:] = np.float32(radius)

    def table():
        return an.calculateAtomRadialProfiles(radius, shells)

    def device():
        return densityObj._map.radial_profiles(xyz, radius, shells, cut)

    def twenty():
        pos = np.stack([densityObj._map.region_sums(xyz, radii[k], off, cut)[0] for k in range(shells)], axis=1)
        return np.diff(pos, axis=1, prepend=0.0)

    forms = {"table_one_call": table, "device_one_call": device, "twenty_region_calls": twenty}
    times = {name: [] for name in forms}
    for rep in range(args.warmup + args.reps):
        for name, fn in forms.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(dt)
    ctx.profile_begin()
    got = device()
    prof = ctx.profile_end()
    curve = twenty()
    top = float(np.abs(dens).max())
    # (the shells of k * w by differencing use float32(k * w) as the region radius: the two curves agree up to voxels on those boundaries)
    out = {"case": args.case, "atoms": n_atoms, "grid": list(ncrs), "radius": radius, "shells": shells, "reps": args.reps,
           "median_ms": {name: round(1e3 * statistics.median(v), 4) for name, v in times.items()},
           "min_ms": {name: round(1e3 * min(v), 4) for name, v in times.items()},
           "kernel_ms": {k: round(ms, 4) for k, (_, ms) in sorted(prof.items())},
           "ratio_twenty_over_device": round(statistics.median(times["twenty_region_calls"]) / statistics.median(times["device_one_call"]), 2),
           "ratio_twenty_over_table": round(statistics.median(times["twenty_region_calls"]) / statistics.median(times["table_one_call"]), 2),
           "voxels_in_spheres": int(got["n"].sum()),
           "total_curve_difference_over_max_rho": float(np.abs(curve.sum(1) - got["sumSig"].sum(1)).max() / top)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
