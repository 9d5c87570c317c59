"""Optimise mode's descent (``optimizeParams.optimize``) against the reference's ``optimizeParams.main`` on a synthetic surface
(tests/golden/make_golden_optimize.py -> optimize_ref.json, Case A): every option set gives the same steps and radii, the same
Testing / Accepted / Rejected lines and the same params files, byte for byte.  Also ``compare`` / ``finalize``, the iteration
cap, invalid input and the sample draw.  CPU only: the surface stands in for the GPU evaluation."""
import json
import os

import pytest

from conftest import GOLDEN
import optimize_surface

LOG_PREFIXES = ("Testing ", "Accepted", "Rejected", "Final Radii:", "Num Accepted Changes=")


def _golden():
    with open(os.path.join(GOLDEN, "optimize_ref.json")) as fh:
        return json.load(fh)


GOLDEN_REF = _golden()
CASE_A = sorted(GOLDEN_REF["case_a"])


def _steps(trace):
    return [{"atomType": s["atomType"], "previousRadius": s["previousRadius"], "radius": s["radius"], "accepted": s["accepted"]} for s in trace]


def _run_case(name, tmp_path, **extra):
    from pdb_eda_amd import optimizeParams
    want = GOLDEN_REF["case_a"][name]
    params = {**optimize_surface.surface_params(), **want["table"]}
    surface = optimize_surface.Surface(params, **want["surface"])
    log, out = str(tmp_path / "run.log"), str(tmp_path / "out.json")
    options = {**want["options"], **extra}
    got = optimizeParams.optimize(params, surface, log=log, outParamsPath=out, **options)
    return want, got, log, out, surface


@pytest.mark.parametrize("name", CASE_A)
def test_descent_matches_reference(name, tmp_path):
    want, (outParams, trace), log, out, surface = _run_case(name, tmp_path)
    assert _steps(trace) == want["steps"]
    assert surface.calls == len(trace) + 1
    with open(log) as fh:
        lines = [ln.rstrip("\n") for ln in fh if ln.startswith(LOG_PREFIXES)]
    assert lines == want["log"]
    with open(out) as fh:
        assert fh.read() == want["out_params"]
    if want["temp_params"] is None:
        assert not os.path.exists(out + ".temp")
    else:
        with open(out + ".temp") as fh:
            assert fh.read() == want["temp_params"]
    assert sum(s["accepted"] for s in trace) == want["accepted"] and sum(not s["accepted"] for s in trace) == want["rejected"]
    assert json.loads(want["out_params"])["radii"] == outParams["radii"]


def test_the_golden_cases_exercise_every_rule():
    """The option sets reach what they are there for: a rejected step, equal penalties (the flat region), many halvings."""
    runs = GOLDEN_REF["case_a"]
    assert all(runs[n]["rejected"] > 0 for n in ("default", "small_min", "flat"))
    assert runs["stop"]["rejected"] == 0 and len(runs["stop"]["steps"]) < len(runs["default"]["steps"])
    assert runs["start_radius"]["steps"][0]["atomType"] == "C.srf.carbonyl" and runs["start_radius"]["steps"][0]["radius"] == 0.95
    assert {s["atomType"] for s in runs["optimize_list"]["steps"]} <= {"C.srf.alpha", "O.srf.carbonyl", "S.srf.thiol"}
    assert not {s["atomType"] for s in runs["optimize_reverse"]["steps"]} & {"C.srf.alpha", "O.srf.carbonyl", "S.srf.thiol"}
    assert len(runs["small_min"]["steps"]) > len(runs["default"]["steps"])


def test_flat_region_accepts_equal_penalties(tmp_path):
    """abs(p) == abs(best) is accepted (<=), with no secant estimate: the flat surface produces such steps."""
    _, (_, trace), _, _, _ = _run_case("flat", tmp_path)
    equal = [s for s in trace if abs(s["penalty"]) == abs(s["bestPenalty"])]
    assert equal and all(s["accepted"] for s in equal)


def test_max_iterations_caps_the_loop(tmp_path):
    want, (outParams, trace), log, out, surface = _run_case("default", tmp_path, maxIterations=4)
    assert len(trace) == 4 and surface.calls == 5
    assert _steps(trace) == want["steps"][:4]
    radii = dict(optimize_surface.surface_params()["radii"])
    for s in trace:
        if s["accepted"]:
            radii[s["atomType"]] = s["radius"]
    assert outParams["radii"] == radii
    with open(out) as fh:
        assert json.load(fh)["radii"] == radii


def test_no_files_without_paths(tmp_path):
    from pdb_eda_amd import optimizeParams
    params = optimize_surface.surface_params()
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        optimizeParams.optimize(params, optimize_surface.Surface(params), maxIterations=3)
    finally:
        os.chdir(cwd)
    assert os.listdir(tmp_path) == []


def test_compare_and_finalize_match_reference(tmp_path):
    from pdb_eda_amd import optimizeParams
    want = GOLDEN_REF["compare_finalize"]
    p1, p2 = json.loads(want["params1"]), json.loads(want["params2"])
    got = optimizeParams.compare(p1, p2, "p1.json", "p2.json")
    assert len(got) == len(want["compare"])
    for g, w in zip(got, want["compare"]):
        if w.startswith("Mean (Std) Radius Differences:"):
            # (the reference sums the differences in set order: the last bit of the mean may differ)
            gm, gs = g.split(": ")[1].replace("(", "").replace(")", "").split()
            wm, ws = w.split(": ")[1].replace("(", "").replace(")", "").split()
            assert float(gm) == pytest.approx(float(wm), rel=1e-12) and float(gs) == pytest.approx(float(ws), rel=1e-12)
        else:
            assert g == w
    for path, p in (("p1.json", p1), ("p2.json", p2)):
        with open(tmp_path / path, "w") as fh:
            json.dump(p, fh)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert optimizeParams.compare("p1.json", "p2.json")[0] == want["compare"][0]
    finally:
        os.chdir(cwd)
    final = optimizeParams.finalize(p1)
    assert "optimize" not in final and "optimize" in p1
    assert optimizeParams.dumpParams(final) == want["finalize"]
    optimizeParams.writeParams(str(tmp_path / "final.json"), final)
    assert (tmp_path / "final.json").read_text() == want["finalize"]


def test_invalid_input_raises(tmp_path):
    from pdb_eda_amd import optimizeParams
    params = optimize_surface.surface_params()
    surface = optimize_surface.Surface(params)
    with pytest.raises(ValueError, match="starting atom"):
        optimizeParams.optimize(params, surface, startAtomType="X.not.a.type")
    with pytest.raises(ValueError, match="does not exist or is not parsable"):
        optimizeParams.optimize(str(tmp_path / "missing.json"), surface)
    (tmp_path / "broken.json").write_text("{not json")
    with pytest.raises(ValueError, match="does not exist or is not parsable"):
        optimizeParams.optimize(str(tmp_path / "broken.json"), surface)
    with pytest.raises(ValueError):
        optimizeParams.optimize({"radii": params["radii"]}, surface)
    with pytest.raises(ValueError):
        optimizeParams.optimize(params, surface, maxIterations=0)
    with pytest.raises(ValueError):
        optimizeParams.optimize(params, surface, minIncrement=0.0)
    with pytest.raises(ValueError, match="not parsable"):
        optimizeParams.compare(str(tmp_path / "missing.json"), params)
    assert surface.calls == 0


def test_sample_draw():
    from pdb_eda_amd import multipleStructures, optimizeParams
    entries = [multipleStructures.Entry("e%02d" % i, None, cost_hint=float(i)) for i in range(20)]
    a = [e.pdbid for e in optimizeParams.sampleEntries(entries, 6, seed=11)]
    b = [e.pdbid for e in optimizeParams.sampleEntries(entries, 6, seed=11, world_size=2)]
    assert a == b and len(set(a)) == 6
    assert [e.pdbid for e in optimizeParams.sampleEntries(entries, 6, seed=12)] != a
    assert optimizeParams.sampleEntries(entries, 0) == entries
    with pytest.raises(ValueError, match="needs a seed"):
        optimizeParams.sampleEntries(entries, 6, seed=None, world_size=2)


def test_entries_from_pdbids(tmp_path):
    import pickle
    from pdb_eda_amd import densityAnalysis, optimizeParams
    (tmp_path / "ccp4_data").mkdir()
    (tmp_path / "ccp4_data" / "1abc.ccp4").write_bytes(b"x" * 100)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        entries = optimizeParams.entriesFromPDBids(["1ABC", "2xyz"])
    finally:
        os.chdir(cwd)
    assert [e.pdbid for e in entries] == ["1abc", "2xyz"] and [e.cost_hint for e in entries] == [100, 0.0]
    loader = pickle.loads(pickle.dumps(entries[0].loader))          # worker processes receive the loader
    assert loader.density_path == str(tmp_path / "ccp4_data" / "1abc.ccp4")
    assert loader.diff_path == str(tmp_path / "ccp4_data" / "1abc_diff.ccp4")
    assert loader.pdb_path == str(tmp_path / "pdb_data" / "pdb1abc.ent.gz")
    assert densityAnalysis.ccp4folder == "./ccp4_data/"
