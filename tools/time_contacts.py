"""Crystal contacts: time of one device call (pdbeda_crystal_contacts: kept images + contacts of every atom, synchronised, after
warm-up) on synthetic P 21 21 21 entries of 2 000 / 10 000 / 50 000 atoms at cutoff 5.0, with the image and neighbour counts; for the
smaller two, the reference's own formulation beside it (scipy cdist over the neighbour list + min per row, in row chunks on a pool of
16 threads) on the same neighbour list.
    python tools/time_contacts.py [--sizes 2000,10000,50000] [--reps 10] [--cpu-max 10000] [--out FILE]
Prints one JSON document."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def entry(n_atoms, seed=21):
    """A P 21 21 21 cell about four times the volume of a box of n_atoms random atoms (protein-like density: ~12 A^3 per atom)."""
    from pdb_eda_amd import ccp4, synthetic
    edge = (12.0 * n_atoms) ** (1.0 / 3.0)
    cell = (2.0 * edge, 1.6 * edge + 4.0, 1.3 * edge + 6.0)
    spec = synthetic.MapSpec(ncrs=(16, 16, 16), cell=cell)
    ortho = np.asarray(ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(spec)).orthoMat, dtype=np.float64)
    oi = np.linalg.inv(ortho)
    ops = [(np.eye(3), (0, 0, 0)), (np.diag([-1, -1, 1]), (0.5, 0, 0.5)), (np.diag([-1, 1, -1]), (0, 0.5, 0.5)), (np.diag([1, -1, -1]), (0.5, 0.5, 0))]
    rot = [np.hstack([np.round(ortho.dot(r).dot(oi), 6) + 0.0, np.round(ortho.dot(t), 5)[:, None] + 0.0]) for r, t in ops]
    rng = np.random.default_rng(seed)
    poly = np.round(rng.uniform(-3.0, edge - 3.0, (n_atoms, 3)), 3)
    return rot, ortho, poly


def reference_formulation(query, neighbours, cutoff, threads=16, chunk=512):
    """findCoordContacts as the reference computes it (cdist + min per row), chunked over rows so the matrix fits in memory."""
    from scipy.spatial.distance import cdist

    def part(s):
        return np.min(cdist(query[s:s + chunk], neighbours), axis=1)
    with ThreadPoolExecutor(threads) as pool:
        mins = np.concatenate(list(pool.map(part, range(0, len(query), chunk))))
    return [(i, d) for i, d in enumerate(mins) if d <= cutoff]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,50000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-max", type=int, default=10000)
    ap.add_argument("--cutoff", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pdb_eda_amd import _native, crystalContacts
    ctx = _native.default_context()
    out = {"cutoff": a.cutoff, "group": "P 21 21 21", "rows": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        rot, ortho, poly = entry(n)
        t0 = time.perf_counter()
        cand = crystalContacts.candidateImages(rot, ortho, poly, a.cutoff)
        t_cand = time.perf_counter() - t0
        for _ in range(2):
            kept, idx, dist = ctx.crystal_contacts(poly, poly, rot, ortho, cand, a.cutoff)
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            kept, idx, dist = ctx.crystal_contacts(poly, poly, rot, ortho, cand, a.cutoff)
            times.append(time.perf_counter() - t0)
        row = {"atoms": n, "candidates": int(len(cand)), "kept_images": int(kept.sum()), "neighbours": int(kept.sum()) * n, "contact_rows": int(len(idx)),
               "candidate_enumeration_ms": round(1e3 * t_cand, 3), "gpu_call_ms_median": round(1e3 * float(np.median(times)), 3),
               "gpu_call_ms_min": round(1e3 * float(np.min(times)), 3)}
        if n <= a.cpu_max:
            neigh = ctx.image_coords(poly, rot, ortho, cand[kept])
            t0 = time.perf_counter()
            ref = reference_formulation(poly, neigh, a.cutoff)
            row["reference_cdist_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            row["reference_rows_equal"] = [i for i, _ in ref] == idx.tolist() and np.array_equal(np.array([d for _, d in ref]), dist)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    text = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
