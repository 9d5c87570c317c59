"""Atom Q-scores (pdbeda_atom_qscores) and the trilinear read (pdbeda_interp_density) against the host route a user would write
without them: scipy.ndimage.map_coordinates(order=1, mode='grid-wrap') for the values and a cKDTree for "is this atom the nearest
one" (where scipy is missing: numpy gathers and a brute-force distance table).  Two workloads over the 2Fo-Fc map:

  analysis_128  bench.py's analysis entry: 128^3, 2 000 atoms, all symmetry atoms competing, the identity images scored;
  bench_256     a 256^3 map (the size of bench.py's flagship map) with 50 000 atoms at bond-length spacing, all scored.

One `DensityMatrix.qScores` call per repetition with the defaults (21 shells of 0.1 A, lattices of 8 .. 64 directions); medians
after warm-up.  The host route is timed on at most --host-atoms scored atoms (all atoms still compete) and reported per atom beside
the device's; its scores are compared with the device's (they differ where the host's nearest-atom query breaks an exact tie the
other way, and by rounding).  --only-device leaves the host route out (a profiler run of the new kernels).  The figures are written
into DESIGN.md 4.11."""
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
    """``n`` atoms: a random walk of ``bond``-long steps folded back into the box [lo, hi]."""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n, 3))
    steps *= bond / np.linalg.norm(steps, axis=1)[:, None]
    steps[0] = rng.uniform(0.0, hi - lo)
    span = hi - lo
    pos = np.mod(np.cumsum(steps, axis=0), 2.0 * span)
    return lo + np.where(pos > span, 2.0 * span - pos, pos)


def host_route(header, grid, xyz, scored, step, ref, unit, offsets, min_points):
    """The Q-scores of ``scored`` on the host: level by level, only the shells that have not stopped yet."""
    try:
        from scipy.ndimage import map_coordinates
        from scipy.spatial import cKDTree
        tree = cKDTree(xyz)
    except ImportError:
        map_coordinates = tree = None
    shells = len(ref)
    radii = np.arange(shells) * float(np.float32(step))
    origin, length = np.asarray(header.origin, dtype=np.float64), np.asarray(header.gridLength, dtype=np.float64)

    def sample(points):          # (orthogonal maps that store their whole cell: the tool's own)
        f = (points - origin) / length
        crs = np.stack([f[:, header.map2crs[j]] for j in range(3)], axis=0)
        if map_coordinates is not None:
            return map_coordinates(grid, crs[::-1], order=1, mode="grid-wrap")
        base = np.floor(crs)
        t, b = crs - base, base.astype(np.int64)
        n = np.array(grid.shape[::-1])[:, None]
        out = np.zeros(points.shape[0])
        for k in range(8):
            d = np.array([k & 1, (k >> 1) & 1, k >> 2])[:, None]
            w = np.prod(np.where(d == 1, t, 1.0 - t), axis=0)
            i = np.mod(b + d, n)
            out += w * grid[i[2], i[1], i[0]]
        return out

    def nearest_is(points, owner):
        if tree is not None:
            dist, idx = tree.query(points, k=1, workers=-1)
            own = np.linalg.norm(points - xyz[owner], axis=1)
            return (idx == owner) | (dist >= own)
        own = ((points - xyz[owner]) ** 2).sum(axis=1)
        keep = np.ones(len(points), dtype=bool)
        for lo in range(0, len(xyz), 256):
            d = ((points[:, None, :] - xyz[None, lo:lo + 256, :]) ** 2).sum(axis=2)
            keep &= ~((d < own[:, None]) & (np.arange(lo, min(lo + 256, len(xyz)))[None, :] != owner[:, None])).any(axis=1)
        return keep

    q = np.full(len(scored), np.nan)
    n_points = np.ones(len(scored), dtype=np.int64)
    sums = np.zeros((5, len(scored)))          # x, xx, y, yy, xy over the kept points (x shifted by the atom's own sample)
    v0 = sample(xyz[scored])
    open_atom, open_shell = [a.reshape(-1) for a in np.meshgrid(np.arange(len(scored)), np.arange(1, shells), indexing="ij")]
    for l in range(len(offsets) - 1):
        if len(open_atom) == 0:
            break
        u = unit[offsets[l]:offsets[l + 1]]
        pts = (xyz[scored][open_atom][:, None, :] + radii[open_shell][:, None, None] * u[None, :, :]).reshape(-1, 3)
        keep = nearest_is(pts, np.repeat(scored[open_atom], len(u))).reshape(-1, len(u))
        done = (keep.sum(axis=1) >= min_points) | (l == len(offsets) - 2)
        rows = np.nonzero(done)[0]
        mask = keep[rows].reshape(-1)
        atom = np.repeat(open_atom[rows], len(u))[mask]
        shell = np.repeat(open_shell[rows], len(u))[mask]
        x = sample(pts.reshape(-1, len(u), 3)[rows].reshape(-1, 3)[mask]) - v0[atom]
        y = ref[shell] - ref[0]
        for k, term in enumerate((x, x * x, y, y * y, x * y)):
            sums[k] += np.bincount(atom, weights=term, minlength=len(scored))
        n_points += np.bincount(atom, minlength=len(scored))
        open_atom, open_shell = open_atom[~done], open_shell[~done]
    n = n_points.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov, vx, vy = sums[4] - sums[0] * sums[2] / n, sums[1] - sums[0] ** 2 / n, sums[3] - sums[2] ** 2 / n
        q = np.clip(cov / (np.sqrt(vx) * np.sqrt(vy)), -1.0, 1.0)
    return q, n_points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-atoms", type=int, default=5000)
    ap.add_argument("--workloads", default="analysis_128,bench_256")
    ap.add_argument("--only-device", action="store_true")
    args = ap.parse_args()
    from pdb_eda_amd import _native, ccp4, synthetic, structure, densityAnalysis as da
    ctx = _native.default_context()
    ref, unit, offsets = ccp4.qScoreTables()
    for name in args.workloads.split(","):
        if name == "analysis_128":
            spec, header, st, params, dens, diff, rot = synthetic.cube_entry((128, 128, 128), 400, 5, 0.5)
            da.setGlobals(params)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), "synth", ctx=ctx)
            diffObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), "synth", ctx=ctx)
            da._attachCutoffs(dm, diffObj)
            an = da.DensityAnalysis("synth", dm, diffObj, st, structure.PDBEntry(structure.PDBHeader(pdbid="synth", resolution=2.0, spaceGroup="P_1", rotationMats=rot)))
            xyz = np.ascontiguousarray(an.symmetryAtomCoords, dtype=np.float64)
            scored = np.nonzero(an.symmetryAtoms._ident)[0].astype(np.int32)
            grid = np.asarray(dens, dtype=np.float32).reshape(128, 128, 128)
        else:
            spec = synthetic.MapSpec(ncrs=(256, 256, 256), spacing=0.5)
            grid = synthetic.noise_grid(spec, seed=9, sigma_voxels=1.5)
            dm = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, grid)), "synth", ctx=ctx)
            xyz = walk(50000, np.zeros(3), np.full(3, 127.5), seed=21)
            scored = np.arange(len(xyz), dtype=np.int32)
        header = dm.header
        times = {"qscores": [], "interp_density_of_the_atoms": [], "host_route": []}
        for rep in range(args.warmup + args.reps):
            for k, fn in (("qscores", lambda: dm.qScores(xyz, scored=scored)), ("interp_density_of_the_atoms", lambda: dm.getInterpolatedDensityFromXyz(xyz))):
                ctx.synchronize()
                t0 = time.perf_counter()
                got = fn()
                if rep >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        got = dm.qScores(xyz, scored=scored)
        host_n, worst, same_points = 0, None, None
        if not args.only_device:
            pick = np.arange(len(scored)) if len(scored) <= args.host_atoms else np.sort(np.random.default_rng(1).choice(len(scored), args.host_atoms, replace=False))
            host_n = len(pick)
            for rep in range(args.host_reps):
                t0 = time.perf_counter()
                q, n_points = host_route(header, grid, xyz, scored[pick].astype(np.int64), 0.1, ref, unit, offsets.tolist(), 8)
                times["host_route"].append(time.perf_counter() - t0)
            both = np.isfinite(q) & np.isfinite(got["q"][pick]) & (n_points == got["nPoints"][pick])
            same_points = int((n_points == got["nPoints"][pick]).sum())
            worst = float(np.abs(q[both] - got["q"][pick][both]).max()) if both.any() else None
        ctx.profile_begin()
        dm.qScores(xyz, scored=scored)
        prof = {k: round(ms, 4) for k, (_, ms) in sorted(ctx.profile_end().items())}
        med = {k: round(1e3 * statistics.median(v), 4) for k, v in times.items() if v}
        have = np.isfinite(got["q"])
        out = {"workload": name, "grid": [int(v) for v in header.ncrs], "competing_atoms": len(xyz), "scored_atoms": len(scored), "reps": args.reps, "median_ms": med,
               "min_ms": {k: round(1e3 * min(v), 4) for k, v in times.items() if v}, "kernel_ms": prof, "counters": got["counters"].tolist(),
               "sample_points": int(got["nPoints"].sum()), "atoms_with_a_score": int(have.sum()), "mean_q": round(float(got["q"][have].mean()), 4),
               "host_route_atoms": host_n, "host_atoms_with_the_same_points": same_points, "host_max_abs_q_difference_where_the_points_agree": worst,
               "us_per_atom": {"qscores": round(1e3 * med["qscores"] / len(scored), 3), "host_route": round(1e3 * med["host_route"] / host_n, 3) if host_n else None}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
