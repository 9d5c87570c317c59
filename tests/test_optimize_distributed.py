"""Optimise mode's descent over two ranks on CPU (gloo): every rank runs the same decisions on the same all-gathered
reduction (``optimizeStats.calculateMedianDiffsSlopes``), ends with the same parameter table as a single-process run, and only
rank 0 writes files; a rank that fails makes both ranks raise instead of hanging."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per-entry records as smooth functions of the current radii (a stand-in for the GPU re-analysis of resident entries), reduced
# over ALL ranks by the real statistics path.
EVALUATOR = r'''
import math
from pdb_eda_amd import multipleStructures, optimizeStats, synthetic

def make_entries(n=11):
    return [multipleStructures.Entry("e%02d" % i, None, cost_hint=float((7 * i) % n)) for i in range(n)]

class FakeSweep(object):
    def __init__(self, entries, fail_at=None):
        self.entries, self.fail_at, self.calls = entries, fail_at, 0

    def record(self, entry, params):
        k = int(entry.pdbid[1:])
        types = list(params["radii"])
        diffs, comp, inc = {}, {}, {}
        for i, t in enumerate(types):
            if (k + i) % 5 == 4:
                continue                        # this entry has no atom of type t
            r = params["radii"][t]
            diffs[t] = (1.1 + 0.2 * i) * (r - (0.8 + 0.03 * ((i * 3) % 5))) + 0.013 * math.sin(3.1 * k + i)
            c = int(round(40.0 / (1.0 + math.exp(-8.0 * (r - 0.76)))))
            comp[t], inc[t] = c, 40 - c + (k % 3)
        return {"pdbid": entry.pdbid, "diffs": diffs, "slopes": {t: -0.5 - 0.01 * k for t in diffs},
                "atomtype_overlap_completeness": comp, "atomtype_overlap_incompleteness": inc}

    def iteration(self, params):
        self.calls += 1
        error = RuntimeError("device lost on this rank") if self.calls == self.fail_at else None
        records = [] if error else [self.record(e, params) for e in self.entries]
        optimizeStats.all_ranks_ok(error)
        return optimizeStats.calculateMedianDiffsSlopes(records, params), records

def start_params():
    return {**synthetic.synthetic_params(), "optimize": ["C.syn.methyl", "O.syn.carbonyl", "N.syn.amide", "C.syn.alpha"]}

OPTIONS = dict(maxIncrement=0.1, minIncrement=0.002)
'''

WORKER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
exec(open(%(evaluator)r).read())
from pdb_eda_amd import multipleStructures, optimizeParams
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=2)
mine = multipleStructures.shard(make_entries(), rank, 2)
where = os.path.join(%(out)r, "rank%%d" %% rank)
os.makedirs(where)
fail_at = %(fail_at)r if rank == 1 else None
try:
    outParams, trace = optimizeParams.optimize(start_params(), FakeSweep(mine, fail_at), log=os.path.join(where, "run.log"),
                                               outParamsPath=os.path.join(where, "out.json"), **OPTIONS)
    outcome = {"radii": outParams["radii"], "slopes": outParams["slopes"], "steps": [[s["atomType"], s["radius"], s["accepted"]] for s in trace]}
except Exception as e:
    outcome = {"error": "%%s: %%s" %% (type(e).__name__, e)}
with open(os.path.join(%(out)r, "outcome%%d.json" %% rank), "w") as fh:
    json.dump(outcome, fh)
dist.destroy_process_group()
'''


def _two_ranks(tmp_path, port, fail_at=None):
    evaluator = tmp_path / "evaluator.py"
    evaluator.write_text(EVALUATOR)
    out = tmp_path / "out"
    out.mkdir()
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(root=ROOT, evaluator=str(evaluator), port=port, out=str(out), fail_at=fail_at))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)]) for r in range(2)]
    try:
        codes = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0]
    return out, [json.loads((out / ("outcome%d.json" % r)).read_text()) for r in range(2)]


def _single_process(tmp_path):
    namespace = {}
    exec(EVALUATOR, namespace)
    from pdb_eda_amd import optimizeParams
    outParams, trace = optimizeParams.optimize(namespace["start_params"](), namespace["FakeSweep"](namespace["make_entries"]()),
                                               outParamsPath=str(tmp_path / "single.json"), **namespace["OPTIONS"])
    return outParams, trace


def test_two_ranks_decide_alike_and_only_rank0_writes(tmp_path):
    out, (r0, r1) = _two_ranks(tmp_path, 33500 + os.getpid() % 2000)
    assert "error" not in r0 and "error" not in r1
    assert r0 == r1
    single, trace = _single_process(tmp_path)
    assert r0["radii"] == single["radii"] and r0["slopes"] == single["slopes"]
    assert r0["steps"] == [[s["atomType"], s["radius"], s["accepted"]] for s in trace]
    assert len(trace) > 3 and any(s["accepted"] for s in trace) and any(not s["accepted"] for s in trace)
    assert sorted(os.listdir(out / "rank0")) == ["out.json", "out.json.temp", "run.log"]
    assert os.listdir(out / "rank1") == []
    assert json.loads((out / "rank0" / "out.json").read_text())["radii"] == single["radii"]
    assert (out / "rank0" / "out.json").read_text() == (tmp_path / "single.json").read_text()


def test_a_failing_rank_ends_the_descent_on_both_ranks(tmp_path):
    """Rank 1's third evaluation fails: both ranks leave the descent with an error (no hang in the all-gather)."""
    _, (r0, r1) = _two_ranks(tmp_path, 35500 + os.getpid() % 2000, fail_at=3)
    assert r1["error"] == "RuntimeError: device lost on this rank"
    assert r0["error"].startswith("RuntimeError: another rank failed")
