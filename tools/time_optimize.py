"""What one iteration of optimise mode's descent costs: synthetic entries written as CCP4 files and loaded as files (resident in
HBM), then ``optimizeParams.optimize`` capped at ``--iterations`` loop steps, once over a thread ``Sweep`` and once over a
``ProcessSweep``.  Prints one JSON line per mode: load time, total descent wall time, ms per evaluation, ms per entry-evaluation.

    python tools/time_optimize.py [--entries 32] [--files 4] [--edge 200] [--residues 100] [--workers 4] [--iterations 10]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402
from pdb_eda_amd import multipleStructures, optimizeParams, optimizeSweep, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=32)
    ap.add_argument("--files", type=int, default=4, help="distinct entry files; the entries reuse them in turn")
    ap.add_argument("--edge", type=int, default=200)
    ap.add_argument("--residues", type=int, default=100)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=10)
    a = ap.parse_args()
    params = {**synthetic.synthetic_params(), "optimize": ["C.syn.methyl", "O.syn.carbonyl", "N.syn.amide"]}
    tmp = tempfile.mkdtemp(prefix="pdbeda_time_optimize_")
    try:
        loaders = [synthetic.write_entry_files(tmp, "e%d" % k, a.edge, a.residues, 40 + k, as_paths=True) for k in range(a.files)]
        entries = [multipleStructures.Entry("e%04d" % i, loaders[i % a.files]) for i in range(a.entries)]
        for mode in ("threads", "processes"):
            t0 = time.perf_counter()
            sweep = optimizeSweep.ProcessSweep(entries, 0, a.workers) if mode == "processes" else optimizeSweep.Sweep(entries, 0, a.workers)
            t_load = time.perf_counter() - t0
            try:
                t0 = time.perf_counter()
                _, trace = optimizeParams.optimize(params, sweep, maxIncrement=0.05, minIncrement=0.001, maxIterations=a.iterations)
                t_descent = time.perf_counter() - t0
            finally:
                sweep.close()
            evaluations = len(trace) + 1           # the start evaluation + one per loop step
            print(json.dumps({"mode": mode, "workers": a.workers, "entries": a.entries, "edge": a.edge, "residues": a.residues,
                              "evaluations": evaluations, "accepted": sum(s["accepted"] for s in trace),
                              "load_s": round(t_load, 3), "descent_s": round(t_descent, 3),
                              "ms_per_iteration": round(1e3 * t_descent / evaluations, 2),
                              "ms_per_entry_iteration": round(1e3 * t_descent / evaluations / a.entries, 3)}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
