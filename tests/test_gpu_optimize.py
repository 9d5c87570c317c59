"""Optimise mode end to end on the MI355X: ``optimizeParams.run`` replays golden Case B (tests/golden/make_golden_optimize.py ->
optimize_ref.json: the reference's ``optimizeParams.main`` with its own ``calculateMedianDiffsSlopes`` on the three synthetic
analysis entries) with worker processes and with threads.  Steps and accept / reject choices identical, radii within 1e-9,
medians and penalties within 1e-7 relative (the recorded decision margins are far wider)."""
import json
import os

import pytest

from conftest import GOLDEN, ANALYSIS_CASES, load_analysis_case

pytestmark = pytest.mark.gpu
REL = 1e-7


class AnalysisCaseLoader(object):
    """Loader of one golden analysis entry; picklable, so the worker processes of a ProcessSweep rebuild it themselves."""

    def __init__(self, name):
        self.name = name

    def __call__(self):
        from pdb_eda_amd import synthetic
        z, spec, st, pdb, _ = load_analysis_case(self.name)
        return synthetic.ccp4_bytes(spec, z["dens"]), synthetic.ccp4_bytes(spec, z["diff"]), st, pdb


def _golden():
    with open(os.path.join(GOLDEN, "optimize_ref.json")) as fh:
        return json.load(fh)["case_b"]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("processes", [True, False], ids=["processes", "threads"])
def test_descent_replays_reference(processes, tmp_path):
    from pdb_eda_amd import multipleStructures, optimizeParams
    want = _golden()
    assert want["ids"] == ANALYSIS_CASES
    entries = [multipleStructures.Entry(name, AnalysisCaseLoader(name)) for name in ANALYSIS_CASES]
    out, log = str(tmp_path / "out.json"), str(tmp_path / "run.log")
    outParams, trace = optimizeParams.run(want["params"], entries, device=0, workers=2, processes=processes,
                                          log=log, outParamsPath=out, **want["options"])
    assert [(s["atomType"], s["accepted"]) for s in trace] == [(s["atomType"], s["accepted"]) for s in want["steps"]]
    for got, w, ev in zip(trace, want["steps"], want["evaluations"][1:]):
        assert got["previousRadius"] == pytest.approx(w["previousRadius"], abs=1e-9, rel=0)
        assert got["radius"] == pytest.approx(w["radius"], abs=1e-9, rel=0)
        assert got["medianDiffs"].keys() == ev["medianDiffs"].keys()
        for t in ev["medianDiffs"]:
            assert got["medianDiffs"][t] == pytest.approx(ev["medianDiffs"][t], rel=REL, abs=1e-12), (t, got["atomType"])
            assert got["penalties"][t] == pytest.approx(ev["penalties"][t], rel=REL, abs=1e-12), (t, got["atomType"])
    wantParams = json.loads(want["out_params"])
    for t, r in wantParams["radii"].items():
        assert outParams["radii"][t] == pytest.approx(r, abs=1e-9, rel=0)
    assert outParams["slopes"] == wantParams["slopes"]            # the table's own slopes win (ref 165, 260)
    with open(out) as fh:
        written = json.load(fh)
    assert written["radii"] == outParams["radii"] and written["optimize"] == want["params"]["optimize"]
    final = optimizeParams.finalize(out)
    assert "optimize" not in final and final["radii"] == written["radii"]
    with open(log) as fh:
        lines = [ln for ln in fh if ln.startswith(("Accepted", "Rejected"))]
    assert len(lines) == len(want["steps"]) and sum(ln.startswith("Accepted") for ln in lines) == want["accepted"]
