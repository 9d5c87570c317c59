"""pdbeda_pose_scores on the MI355X path against tests/pose_checker.py, the plain numpy restatement of the contract in include/pdbeda.h: the score
table as BYTES, the low-atom counts, the kept flags, the ranked rows and the kept counts with ==, the counters against the plan's restatement;
the staged and the global path on the same input to the byte; two calls, permuted centres, permuted rotations, full against ranked-only; and
every refusal, after which the context stays usable.  The checker's table of a case is computed once and shared."""
import io

import numpy as np
import pytest

import pose_cases as cases
import pose_checker as checker

pytestmark = pytest.mark.gpu

_maps, _wanted = {}, {}
CASES = cases.all_cases()
IDS = [c["tag"] for c in CASES]


def device_map(name, gpu_ctx):
    from pdb_eda_amd import ccp4
    if name not in _maps:
        _maps[name] = ccp4.parse(io.BytesIO(cases.map_bytes(name)), name, ctx=gpu_ctx)
    return _maps[name]


def wanted(case):
    if case["tag"] not in _wanted:
        _wanted[case["tag"]] = checker.scores(cases.header_of(case["map"]), cases.grid_of(case["map"]), case["frag"], case["w"], case["rot"], case["centres"],
                                              case["floor"], case["max_low"], case["allow_outside"])
    return _wanted[case["tag"]]


def call(dm, case, **kw):
    args = dict(topK=case["top_k"], floor=case["floor"], maxLow=case["max_low"], allowOutside=case["allow_outside"], full=True)
    args.update(kw)
    return dm.poseScores(case["frag"], case["w"], case["rot"], case["centres"], **args)


def same_table(a, b):
    return (a["scores"].tobytes() == b["scores"].tobytes() and np.array_equal(a["low"], b["low"]) and np.array_equal(a["kept"], b["kept"])
            and same_rows(a, b))


def same_rows(a, b):
    return (np.array_equal(a["bestRot"], b["bestRot"]) and a["bestScore"].tobytes() == b["bestScore"].tobytes() and np.array_equal(a["bestLow"], b["bestLow"])
            and np.array_equal(a["nKept"], b["nKept"]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_checker(gpu_ctx, case):
    dm = device_map(case["map"], gpu_ctx)
    want = wanted(case)
    got = call(dm, case)
    rot, score, low, n_kept = checker.ranking(want, case["top_k"])
    print("%s: %d centres x %d rotations x %d atoms, kept %d, rejected %d, counters %s"
          % (case["tag"], len(case["centres"]), len(case["rot"]), len(case["frag"]), int(want["kept"].sum()), int((~want["kept"]).sum()), got["counters"]))
    assert got["scores"].dtype == np.float64 and got["scores"].shape == want["scores"].shape
    assert got["scores"].tobytes() == want["scores"].tobytes(), case["tag"]
    assert got["low"].dtype == np.int32 and np.array_equal(got["low"], want["low"]), case["tag"]
    assert np.array_equal(got["kept"], want["kept"]), case["tag"]
    assert got["bestRot"].dtype == np.int32 and np.array_equal(got["bestRot"], rot), case["tag"]
    assert got["bestScore"].tobytes() == score.tobytes(), case["tag"]
    assert np.array_equal(got["bestLow"], low) and np.array_equal(got["nKept"], n_kept), case["tag"]
    assert got["counters"] == checker.counters(cases.header_of(case["map"]), case["frag"], case["centres"], want["kept"]), case["tag"]
    # the two paths on the same input: the same bytes, and the counters say which ran
    direct = dm._map.pose_scores(case["frag"], case["w"], case["rot"], case["centres"], case["top_k"], case["floor"], case["max_low"], case["allow_outside"], True, global_only=True)
    assert same_table(direct, got), case["tag"]
    assert direct["counters"] == checker.counters(cases.header_of(case["map"]), case["frag"], case["centres"], want["kept"], global_only=True), case["tag"]
    assert direct["counters"]["globalCentres"] == len(case["centres"]) and direct["counters"]["maxStagedBox"] == 0
    # two calls: the same bytes; without the tables: the same rows
    assert same_table(call(dm, case), got), case["tag"]
    short = call(dm, case, full=False)
    assert "scores" not in short and same_rows(short, got) and short["counters"] == got["counters"], case["tag"]


def test_the_staging_edge_takes_the_path_the_plan_says(gpu_ctx):
    fits, exceeds, fine = (call(device_map(cases.find(tag)["map"], gpu_ctx), cases.find(tag)) for tag in ("stage-fits", "stage-exceeds", "fine-wraps"))
    assert fits["counters"]["globalCentres"] == 0 and fits["counters"]["maxStagedBox"] == 31 ** 3
    assert exceeds["counters"]["globalCentres"] == 2 and exceeds["counters"]["maxStagedBox"] == 0
    assert fine["counters"]["globalCentres"] == 0 and fine["counters"]["maxStagedBox"] > 24 ** 3


@pytest.mark.parametrize("tag", ["orth-7-257", "hex-7-257", "cut-7-65", "nan-7-64"])
def test_permuted_centres_permute_the_rows(gpu_ctx, tag):
    case = cases.find(tag)
    dm = device_map(case["map"], gpu_ctx)
    got = call(dm, case)
    perm = np.random.default_rng(29).permutation(len(case["centres"]))
    moved = dm.poseScores(case["frag"], case["w"], case["rot"], case["centres"][perm], topK=case["top_k"], floor=case["floor"], maxLow=case["max_low"],
                          allowOutside=case["allow_outside"], full=True)
    for key in ("scores", "low", "kept", "bestRot", "bestScore", "bestLow", "nKept"):
        assert moved[key].tobytes() == got[key][perm].tobytes(), (tag, key)
    assert moved["counters"] == got["counters"]


@pytest.mark.parametrize("tag", ["orth-7-257", "hex-65-65", "weights-7-65"])
def test_permuted_rotations_map_the_winners(gpu_ctx, tag):
    """rot' = rot[perm]: the tables' columns move with the rotations, and wherever a centre's ranked scores are distinct bestRot' = inverse(perm)[bestRot]."""
    case = cases.find(tag)
    dm = device_map(case["map"], gpu_ctx)
    got = call(dm, case)
    perm = np.random.default_rng(31).permutation(len(case["rot"]))
    inverse = np.argsort(perm)
    moved = dm.poseScores(case["frag"], case["w"], case["rot"][perm], case["centres"], topK=case["top_k"], floor=case["floor"], maxLow=case["max_low"],
                          allowOutside=case["allow_outside"], full=True)
    assert moved["scores"].tobytes() == got["scores"][:, perm].tobytes() and np.array_equal(moved["kept"], got["kept"][:, perm])
    assert moved["bestScore"].tobytes() == got["bestScore"].tobytes() and np.array_equal(moved["nKept"], got["nKept"])
    checked = 0
    for c in range(len(case["centres"])):
        filled = got["bestRot"][c] >= 0
        s = got["bestScore"][c][filled]
        distinct = np.ones(len(s), dtype=bool)
        distinct[1:] &= s[1:] != s[:-1]
        distinct[:-1] &= s[:-1] != s[1:]
        assert np.array_equal(moved["bestRot"][c][filled][distinct], inverse[got["bestRot"][c][filled][distinct]]), (tag, c)
        checked += int(distinct.sum())
    assert checked > 0


def test_equal_scores_go_to_the_lower_index(gpu_ctx):
    """The identity listed twice: rotations 0 and 1 score the same bits at every centre and 0 is ranked directly before 1; every atom on the pivot: every
    rotation ties and the rows are 0, 1, 2, ..."""
    case = cases.find("centro-8-7")
    got = call(device_map(case["map"], gpu_ctx), case)
    assert got["scores"][:, 0].tobytes() == got["scores"][:, 1].tobytes()
    for row in got["bestRot"]:
        at = row.tolist().index(0)
        assert row[at + 1] == 1
    pivot = cases.find("pivot-3-64")
    got = call(device_map(pivot["map"], gpu_ctx), pivot)
    kept_rows = got["nKept"] > 0
    assert kept_rows.any() and np.all(got["bestRot"][kept_rows] == np.arange(pivot["top_k"]))
    assert np.all(got["bestRot"][~kept_rows] == -1) and not np.any(got["bestScore"][~kept_rows].view(np.uint64))      # -1 and +0.0 to the bit


def test_a_large_call_is_cut_into_chunks_with_the_same_rows(gpu_ctx):
    """2 ** 20 rotations (the cap): the table of one centre takes 13 MiB and four centres fill a chunk; five centres take two launches.  Every row equals
    the row of the same centre alone."""
    case = cases.find("orth-1-1")
    dm = device_map("orth", gpu_ctx)
    rot = np.tile(np.eye(3), (checker.MAX_ROTATIONS, 1, 1))
    rot[5::7] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    frag, w = cases.fragment(2)
    centres = case["centres"][:5]
    assert checker.chunk(len(centres), len(rot)) == 4
    got = dm.poseScores(frag, w, rot, centres, topK=3)
    alone = dm.poseScores(frag, w, rot, centres[4:5], topK=3)
    assert all(got[k][4:5].tobytes() == alone[k].tobytes() for k in ("bestRot", "bestScore", "bestLow", "nKept"))
    small = dm.poseScores(frag, w, rot[:14], centres, topK=3, full=True)
    assert np.all(np.isin(got["bestRot"], (0, 1, 2, 5, 12, 19))) and np.all(got["nKept"] == checker.MAX_ROTATIONS)
    assert np.array_equal(np.sort(got["bestScore"][:, 0]), np.sort(small["scores"].max(axis=1)))


def test_refusals_leave_the_context_usable(gpu_ctx):
    """Every refusal of the contract raises PDBEDA_ERR_ARGUMENT and the next call computes the same bytes."""
    from pdb_eda_amd import _native
    case = cases.find("orth-7-257")
    dm = device_map(case["map"], gpu_ctx)
    good = call(dm, case)
    frag, w, rot, centres = case["frag"], case["w"], case["rot"], case["centres"]

    def refused(fn):
        with pytest.raises(_native.PdbedaError) as info:
            fn()
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT
        assert same_table(call(dm, case), good)

    def with_value(array, at, value):
        out = np.array(array, dtype=np.float64, copy=True)
        out.reshape(-1)[at] = value
        return out

    refused(lambda: dm.poseScores(np.zeros((checker.MAX_ATOMS + 1, 3)), np.ones(checker.MAX_ATOMS + 1), rot, centres))        # the limits
    refused(lambda: dm.poseScores(np.zeros((0, 3)), np.zeros(0), rot, centres))
    refused(lambda: dm.poseScores(frag, w, np.zeros((0, 3, 3)), centres))
    refused(lambda: dm.poseScores(frag, w, rot, centres, topK=0))
    refused(lambda: dm.poseScores(frag, w, rot, centres, topK=checker.MAX_TOP + 1))
    for bad in (np.nan, np.inf, -np.inf):
        refused(lambda: dm.poseScores(with_value(frag, 4, bad), w, rot, centres))                                          # non-finite inputs
        refused(lambda: dm.poseScores(frag, with_value(w, 2, bad), rot, centres))
        refused(lambda: dm.poseScores(frag, w, with_value(rot, 13, bad), centres))
        refused(lambda: dm.poseScores(frag, w, rot, with_value(centres, 7, bad)))
    refused(lambda: dm.poseScores(frag, w, rot, with_value(centres, 7, 3.0e8)))                                             # 2^29 grid steps of 0.5 A or more
    refused(lambda: dm.poseScores(with_value(frag, 4, 3.0e8), w, rot, centres))                                             # the fragment's reach
    lib, h = dm._ctx._lib, dm._map._h
    ptr = lambda a: _native._ptr(np.ascontiguousarray(a, dtype=np.float64))
    refused(lambda: dm._ctx.check(lib.pdbeda_pose_scores(h, ptr(frag), ptr(w), len(frag), ptr(rot), len(rot), ptr(centres), len(centres), 0.0, 0, 1, 4,
                                                         None, None, None, None, None, None, None, None), "pdbeda_pose_scores"))          # an unknown flag
    refused(lambda: dm._ctx.check(lib.pdbeda_pose_scores(h, ptr(frag), ptr(w), len(frag), ptr(rot), len(rot), ptr(centres), 2 ** 31 // len(rot) + 1, 0.0, 0, 1, 0,
                                                         None, None, None, None, None, None, None, None), "pdbeda_pose_scores"))          # 2^31 poses (refused before the centres are read)
    # the empty call succeeds and touches nothing; every output may be NULL
    ctr = np.full(3, 7, dtype=np.int64)
    assert lib.pdbeda_pose_scores(h, ptr(frag), ptr(w), len(frag), ptr(rot), len(rot), None, 0, 0.0, 0, 1, 0, None, None, None, None, None, None, None, _native._ptr(ctr)) == 0
    assert np.all(ctr == 7)
    assert lib.pdbeda_pose_scores(h, ptr(frag), ptr(w), len(frag), ptr(rot), len(rot), ptr(centres), len(centres), 0.0, 0, 1, 0, None, None, None, None, None, None, None, None) == 0
    empty = dm.poseScores(frag, w, rot, np.zeros((0, 3)), topK=2, full=True)
    assert empty["bestRot"].shape == (0, 2) and empty["scores"].shape == (0, len(rot)) and empty["counters"]["rejected"] == 0
    assert same_table(call(dm, case), good)
