"""Golden record of optimise mode's DESCENT: the reference's ``optimizeParams.main`` run end to end (build container only).

    python tests/golden/make_golden_optimize.py          -> tests/golden/optimize_ref.json

The reference module is loaded through ``refload`` with ``docopt`` stubbed by a prepared argument dict.
  * Case A (synthetic surface): ``calculateMedianDiffsSlopes`` is replaced by ``tests/optimize_surface.Surface`` and ``main()``
    runs once per option set of ``optimize_surface.CASES``.  Kept: the log's Testing / Accepted / Rejected / Final Radii /
    Num Accepted lines, the final and the last ``.temp`` params text, the accept / reject counts.
  * Case B (end to end): the reference's own ``calculateMedianDiffsSlopes`` and ``processFunction`` on the three synthetic
    analysis entries (make_golden_analysis.CASES), ``multiprocessing.Pool`` replaced by a serial stand-in and
    ``densityAnalysis.fromPDBid`` pointed at the reference analyzers.  Kept: the steps, the radii, every evaluation's medians,
    completeness and penalties, and the smallest decision margin (asserted above 1e-5 relative, so that a replay that agrees
    at 1e-7 must make the same decisions).
  * ``--compare`` and ``--finalize`` output for two params files.
Outputs are numbers, names and log text, never reference source.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import refload  # noqa: E402
import optimize_surface  # noqa: E402
from pdb_eda_amd import synthetic  # noqa: E402

LOG_PREFIXES = ("Testing ", "Accepted", "Rejected", "Final Radii:", "Num Accepted Changes=")
CASE_B_TYPES = ["C.syn.methyl", "O.syn.carbonyl", "N.syn.amide"]
CASE_B_OPTIONS = {"maxIncrement": 0.08, "minIncrement": 0.01}
CASE_B_IDS = ["orth", "hex", "alias"]

ARGS = {}


def load_reference():
    ccp4, da = refload.load()
    pkg = sys.modules["pdb_eda"]
    pkg.__version__ = "reference"
    stub = types.ModuleType("docopt")
    stub.docopt = lambda doc, version=None: dict(ARGS)
    sys.modules["docopt"] = stub
    op = importlib.import_module("pdb_eda.optimizeParams")
    op.referenceReduction = op.calculateMedianDiffsSlopes          # (Case A replaces the module's name; Case B needs the original)
    return ccp4, da, op


def args_for(options, **files):
    """The docopt dict of ``pdb_eda optimize`` for optimize()'s keywords."""
    a = {"--help": False, "--ignore": bool(options.get("ignore", False)), "--reverse": bool(options.get("reverse", False)),
         "--sample": "0", "--max": repr(float(options.get("maxIncrement", 0.2))), "--min": repr(float(options.get("minIncrement", 0.001))),
         "--radius": repr(float(options.get("startRadius", 0.0))), "--start": options.get("startAtomType", ""),
         "--stop": repr(float(options.get("stop", 0.0))), "--unweighted": bool(options.get("unweighted", False)),
         "--penalty-weight": repr(float(options.get("inversePenaltyWeight", 3.0))), "--compare": False, "--finalize": False,
         "--testing": False, "<start-params-file>": None, "<pdbid-file>": None, "<log-file>": None, "<out-params-file>": None,
         "<params-file1>": None, "<params-file2>": None}
    a.update(files)
    return a


def run_main(op, tmp, params, options, pdbids):
    start, ids, log, out = (os.path.join(tmp, n) for n in ("start.json", "ids.txt", "run.log", "out.json"))
    for path in (log, out, out + ".temp"):
        if os.path.exists(path):
            os.remove(path)
    with open(start, "w") as fh:
        json.dump(params, fh)
    with open(ids, "w") as fh:
        fh.write("".join(p + "\n" for p in pdbids))
    ARGS.clear()
    ARGS.update(args_for(options, **{"<start-params-file>": start, "<pdbid-file>": ids, "<log-file>": log, "<out-params-file>": out}))
    with contextlib.redirect_stdout(io.StringIO()):
        op.main()
    lines = [ln.rstrip("\n") for ln in open(log)]
    kept = [ln for ln in lines if ln.startswith(LOG_PREFIXES)]
    temp = open(out + ".temp").read() if os.path.exists(out + ".temp") else None
    return {"log": kept, "steps": parse_steps(kept), "out_params": open(out).read(), "temp_params": temp,
            "accepted": sum(1 for ln in kept if ln.startswith("Accepted")), "rejected": sum(1 for ln in kept if ln.startswith("Rejected"))}


def parse_steps(lines):
    steps = []
    for ln in lines:
        if ln.startswith("Testing "):
            atom_type = ln[len("Testing "):].split(" : ")[0].strip()
            start = float(ln.split("starting radius= ")[1].split(" ,")[0])
            radius = float(ln.split("new radius= ")[1].split(" ,")[0])
            steps.append({"atomType": atom_type, "previousRadius": start, "radius": radius})
        elif ln.startswith(("Accepted", "Rejected")):
            steps[-1]["accepted"] = ln.startswith("Accepted")
    return steps


def case_a(op, tmp):
    out = {}
    for name, surface_kw, table, options in optimize_surface.CASES:
        params = {**optimize_surface.surface_params(), **table}
        surface = optimize_surface.Surface(params, **surface_kw)
        op.calculateMedianDiffsSlopes = lambda pdbids, p, testing=False, fn=None, s=surface: s.reduction(p)
        rec = run_main(op, tmp, params, options, ["aaaa"])
        rec.update(name=name, surface=surface_kw, table=table, options=options)
        out[name] = rec
        print("A", name, len(rec["steps"]), "steps", rec["accepted"], "accepted", flush=True)
    return out


class SerialPool(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def starmap(self, fn, iterable, chunksize=1):
        return [fn(*a) for a in iterable]


def case_b(ccp4, da, op, tmp):
    import make_golden_analysis as mga
    from pdb_eda_amd import structure as my_structure
    reduce_ref = op.referenceReduction
    op.multiprocessing = types.SimpleNamespace(Pool=SerialPool)

    def fromPDBid(pdbid):
        name = next(n for n in CASE_B_IDS if n.startswith(pdbid.strip()))        # upstream keeps the first four characters of a line
        spec, st, _, dens, diff, rot = mga.entry(name)
        densityObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), name)
        diffObj = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), name)
        densityObj.densityCutoff = densityObj.meanDensity + 1.5 * densityObj.stdDensity
        diffObj.diffDensityCutoff = diffObj.meanDensity + 3 * diffObj.stdDensity
        pdbObj = my_structure.PDBEntry(my_structure.PDBHeader(pdbid=name, resolution=2.0, spaceGroup="P_1", rotationMats=rot))
        st.header = {"resolution": 2.0}
        return da.DensityAnalysis(name, densityObj, diffObj, st, pdbObj)          # (the globals are processFunction's: not reset)
    da.fromPDBid = fromPDBid

    weight = 3.0
    evaluations = []

    def recording(pdbids, params, testing=False, fn=None):
        result = reduce_ref(pdbids, params, testing, fn)
        median, mean, std, slopes, sizes, completeness = result
        top = max(completeness.values())
        evaluations.append({"radii": dict(params["radii"]), "medianDiffs": {t: float(v) for t, v in median.items()},
                            "overlapCompleteness": {t: float(v) for t, v in completeness.items()},
                            "sizes": {t: int(v) for t, v in sizes.items()},
                            "penalties": {t: float(median[t] + (completeness[t] - top) / weight) for t in median}})
        print("B evaluation", len(evaluations), flush=True)
        return result
    op.calculateMedianDiffsSlopes = recording

    params = {**synthetic.sweep_param_sets()[0], "optimize": list(CASE_B_TYPES)}
    cwd = os.getcwd()
    os.chdir(tmp)                              # processFunction writes its temp JSON files into the working directory
    try:
        rec = run_main(op, tmp, params, dict(CASE_B_OPTIONS), CASE_B_IDS)
    finally:
        os.chdir(cwd)
    rec.update(params=params, options=dict(CASE_B_OPTIONS), ids=CASE_B_IDS, evaluations=evaluations)
    # decision margins: accept / reject (|p| vs |best|) and the choice of the next atom type (top two of |p| * size)
    best = evaluations[0]["penalties"]
    opt = set(CASE_B_TYPES)
    weighted = sorted((abs(best[u] * evaluations[0]["sizes"][u]) for u in best if u in opt), reverse=True)
    margins = [(weighted[0] - weighted[1]) / weighted[0]]
    for step, ev in zip(rec["steps"], evaluations[1:]):
        t = step["atomType"]
        p = ev["penalties"][t]
        margins.append(abs(abs(p) - abs(best[t])) / max(abs(best[t]), 1e-300))
        if step["accepted"]:
            best = ev["penalties"]
        weighted = sorted((abs(best[u]) * ev["sizes"][u] for u in best if u in opt), reverse=True)
        margins.append((weighted[0] - weighted[1]) / weighted[0])
    rec["min_relative_margin"] = min(margins)
    assert rec["min_relative_margin"] > 1e-5, rec["min_relative_margin"]
    print("B", len(rec["steps"]), "steps, min margin", rec["min_relative_margin"], flush=True)
    return rec


def compare_finalize(op, tmp):
    p1 = {**synthetic.sweep_param_sets()[0], "optimize": list(CASE_B_TYPES)}
    p2 = synthetic.sweep_param_sets()[3]
    p2 = {**p2, "radii": {**p2["radii"], "C.syn.alpha": float("nan"), "S.syn.extra": 1.1}, "slopes": {**p2["slopes"], "N.syn.amide": float("nan")}}
    cwd = os.getcwd()
    os.chdir(tmp)                              # relative names: the compare lines name the files
    f1, f2, fo = "p1.json", "p2.json", "final.json"
    for path, p in ((f1, p1), (f2, p2)):
        with open(path, "w") as fh:
            json.dump(p, fh)
    ARGS.clear()
    ARGS.update(args_for({}, **{"--compare": True, "<params-file1>": f1, "<params-file2>": f2}))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        op.main()
    compare = buf.getvalue().splitlines()
    ARGS.clear()
    ARGS.update(args_for({}, **{"--finalize": True, "<start-params-file>": f1, "<out-params-file>": fo}))
    op.main()
    finalized = open(fo).read()
    os.chdir(cwd)
    return {"params1": json.dumps(p1), "params2": json.dumps(p2), "compare": compare, "finalize": finalized}


def main():
    ccp4, da, op = load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        out["case_a"] = case_a(op, tmp)
        out["compare_finalize"] = compare_finalize(op, tmp)
        out["case_b"] = case_b(ccp4, da, op, tmp)
    path = os.path.join(HERE, "optimize_ref.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
