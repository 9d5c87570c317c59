"""The host decisions of pdbeda_aggregate_cloud (pdb_eda_amd/csrc/pdbeda_cloud.h) on a CPU: tests/cloud_harness.cpp, built with the host
compiler under AddressSanitizer + UBSan and -ffp-contract=off (nothing recovered, nothing preloaded, nothing loaded into Python), run as a child
process over a file of cases.  It is the C++ that ships -- the header the library includes -- not a restatement of it.

numpy's sum, std and median, which decide the centroid-distance cut-off, are compared with numpy to the bit.  The pooling step and the finish are
run end to end on every small case of tests/cloud_cases.py and on the flattened inputs of the analysis goldens: the clouds' table comes from
cloud_checker.atom_clouds (the oracle's findAberrantBlobs), what the device would deliver between the two steps from cloud_checker.union_job
(the checker's own components and touches on the pool the harness returned), and the tables must equal cloud_checker.aggregate_cloud.  A sanitizer
report ends the harness with a non-zero status, which fails the test that ran it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import load_analysis_case
import batch_limit_cases
import cloud_cases as cases
import cloud_checker as checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BONDED_KEY_RANGE, COMPONENT_RANGE = 0, 1, 2          # pdbeda_cloud.h: CloudDecision
INT_FIELDS = {"first", "pool_cloud", "pool_atom", "pool_group", "group_res", "pool_voff", "set_off", "pair_a", "pair_b", "pair_owner", "owner_state",
              "atom_idx", "atom_nvox", "res_residue", "res_n", "dom_residue", "dom_n"}


# ---- the harness --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("cloud")
    exe = str(d / "cloud_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pdb_eda_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cloud_harness.cpp"), "-o", exe])
    count = [0]

    def run(records):
        """records: lists of tokens (words, ints, floats).  Returns a dict per output record (pool / finish: "rc" and its arrays; else the value)."""
        count[0] += 1
        case_file, result_file = str(d / ("cases%d.txt" % count[0])), str(d / ("results%d.txt" % count[0]))
        with open(case_file, "w") as f:
            for r in records:
                f.write(" ".join(float(t).hex() if isinstance(t, (float, np.floating)) else str(t) for t in r) + "\n")
        proc = subprocess.run([exe, case_file, result_file], capture_output=True, text=True, timeout=120)
        assert proc.returncode == 0 and proc.stderr == "", proc.stderr[-4000:]
        out = []
        for line in open(result_file):
            t = line.split()
            if t[0] in ("pool", "finish"):
                out.append({"rc": int(t[1])})
            elif t[0] in ("sum", "std", "median", "norm3"):
                out.append(float.fromhex(t[2]))
            else:
                assert int(t[1]) == len(t) - 2, t[0]
                out[-1][t[0]] = np.array([int(x) for x in t[2:]], dtype=np.int64) if t[0] in INT_FIELDS else np.array([float.fromhex(x) for x in t[2:]], dtype=np.float64)
        return out
    return run


def flat(a):
    return list(np.asarray(a).reshape(-1))


def atoms_record(e):
    n, n_keys = len(e["xyz"]), len(e["bonded_off"]) - 1
    return (["atoms", n, n_keys, len(e["owner_key"]), len(e["bonded"])] + flat(np.asarray(e["xyz"], dtype=np.float64)) + flat(np.asarray(e["weight"], dtype=np.float64)) +
            flat(e["residue"]) + flat(e["alias"]) + flat(e["key"]) + (flat(e["bonded_off"]) if n_keys else []) + flat(e["bonded"]) + flat(e["owner_key"]))


def clouds_table(clouds):
    """The sphere job's table as list_stats_one_trip delivers it: a row per cloud, sorted by group (= atom)."""
    rows = [(len(c[0]), c[1], c[2], a) for a, mine in enumerate(clouds) for c in mine]
    return {"n": np.array([r[0] for r in rows], dtype=np.int64), "total": np.array([r[1] for r in rows], dtype=np.float64),
            "centroid": np.array([r[2] for r in rows], dtype=np.float64).reshape(-1, 3), "group": np.array([r[3] for r in rows], dtype=np.int32)}


def clouds_record(t):
    return ["clouds", len(t["n"])] + flat(t["n"]) + flat(t["total"]) + flat(t["centroid"]) + flat(t["group"])


def finish_record(u, min_electrons):
    u_n, u_tot, u_cen, u_grp, comp, touch = u
    return ["finish", len(u_n)] + flat(u_n) + flat(u_tot) + flat(u_cen) + flat(u_grp) + flat(comp) + flat(touch) + [float(min_electrons)]


def check_pool_integers(e, t, p):
    """The integer outputs of the pooling step against a few lines of numpy."""
    n = len(e["xyz"])
    assert np.array_equal(p["first"], np.searchsorted(t["group"], np.arange(n + 1)))
    if len(p["pool_cloud"]) == 0:
        assert all(len(p[f]) == 0 for f in ("pool_atom", "pool_group", "group_res", "pool_voff", "set_off", "pair_a", "pair_b", "pair_owner", "atom_idx"))
        return
    assert np.array_equal(p["pool_voff"], np.concatenate([[0], np.cumsum(t["n"][p["pool_cloud"]])]))
    assert np.array_equal(p["set_off"], np.concatenate([[0], np.cumsum(t["n"])])[p["first"]])
    group_res, pool_group = np.unique(np.asarray(e["residue"])[p["pool_atom"]], return_inverse=True)          # increasing and compact
    assert np.array_equal(p["group_res"], group_res) and np.array_equal(p["pool_group"], pool_group)
    assert np.all(np.diff(p["group_res"]) > 0) and np.all(np.isin(np.diff(p["pool_group"]), (0, 1))) and p["pool_group"][0] == 0
    # the pool: every cloud of every pooled atom's alias, in atom order
    alias = np.asarray(e["alias"])
    want = [(c, i) for i in p["atom_idx"] for c in range(p["first"][alias[i]], p["first"][alias[i] + 1])]
    assert [(int(c), int(i)) for c, i in zip(p["pool_cloud"], p["pool_atom"])] == want
    assert len(p["pair_a"]) == len(p["pair_b"]) == len(p["pair_owner"]) and np.all(np.diff(p["pair_owner"]) >= 0)


def tables_of(p, f):
    """The result dict of DeviceMap.aggregate_cloud from the harness's pool record and (unless nothing was pooled) its finish record."""
    def table(tag):
        if f is None:
            return {"residue": np.zeros(0, np.int32), "total": np.zeros(0), "n": np.zeros(0, np.int64), "electrons": np.zeros(0), "centroid": np.zeros((0, 3))}
        return {"residue": f[tag + "_residue"].astype(np.int32), "total": f[tag + "_total"], "n": f[tag + "_n"], "electrons": f[tag + "_electrons"],
                "centroid": f[tag + "_centroid"].reshape(-1, 3)}
    totals = f["totals"] if f is not None else np.array([0.0, 0.0, 0.0, p["cutoff"][0]])
    assert totals[0] == int(totals[0])
    return {"numVoxels": int(totals[0]), "totalElectrons": float(totals[1]), "totalDensity": float(totals[2]), "centroidDistanceCutoff": float(totals[3]),
            "owner_state": (f if f is not None else p)["owner_state"].astype(np.uint8), "atom": p["atom_idx"].astype(np.int32), "atom_total": p["atom_total"],
            "atom_n": p["atom_nvox"], "atom_centroid": p["atom_centroid"].reshape(-1, 3), "atom_distance": p["atom_dist"], "res": table("res"), "dom": table("dom")}


def decide(harness, header, grid, clouds, e):
    """Both steps of the header on entry e: (the clouds' table, the pool record, the finish record or None, the tables)."""
    t = clouds_table(clouds)
    head = [atoms_record(e), clouds_record(t), ["pool"]]
    p, = harness(head)
    assert p["rc"] == OK
    check_pool_integers(e, t, p)
    if len(p["pool_cloud"]) == 0:          # (where the entry point returns)
        return t, p, None, tables_of(p, None)
    u = checker.union_job(header, grid, clouds, p["pool_cloud"], p["pool_group"], len(p["group_res"]) + 1, p["pair_a"], p["pair_b"])
    p2, f = harness(head + [finish_record(u, e["min_electrons"])])
    assert f["rc"] == OK and all(np.array_equal(p[k], p2[k], equal_nan=True) for k in p if k != "rc")
    return t, p, f, tables_of(p, f)


def want_of(header, grid, clouds, e):
    return checker.aggregate_cloud(header, grid, clouds, *[e[k] for k in cases.ARGS if k != "radius"], e["min_electrons"])


# ---- numpy's sum, std and median to the bit -----------------------------------------------------------------------------------------
LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 20000)          # the pairwise recursion's edges, the 8192-block edges


def wide_values(rng, n):
    """Mixed signs over 40 binades: the order of the additions shows in the last bits."""
    return rng.choice([-1.0, 1.0], size=n) * rng.uniform(1.0, 2.0, size=n) * 2.0 ** rng.integers(-20, 21, size=n)


def test_sum_and_std_equal_numpy_to_the_bit(harness):
    rng = np.random.default_rng(26001)
    xs = [wide_values(rng, n) for n in LENGTHS]
    assert all(n < 64 or np.ptp(np.frexp(x)[1]) >= 30 for n, x in zip(LENGTHS, xs))
    shift = 0.37
    records = []
    for x in xs:
        records += [["sum", 0, 0.0, len(x)] + flat(x), ["sum", 1, shift, len(x)] + flat(x), ["std", len(x)] + flat(x)]
    got = harness(records)
    for k, x in enumerate(xs):
        d = x - shift
        assert got[3 * k] == float(np.add.reduce(x)), len(x)
        assert got[3 * k + 1] == float(np.add.reduce(d * d)), len(x)          # (how np.std sums its squares)
        if len(x) == 0:
            assert np.isnan(got[3 * k + 2])
        else:
            assert got[3 * k + 2] == float(np.std(x)), len(x)
    assert len({float(np.add.reduce(xs[-1])), float(np.sum(np.sort(xs[-1]))), float(sum(xs[-1]))}) > 1          # the order does show on such values


def test_median_equals_numpy_to_the_bit(harness):
    rng = np.random.default_rng(26002)
    xs = [np.zeros(0), np.array([3.25]), np.array([2.0, 1.0]), np.array([1.0, 1e-17]), wide_values(rng, 7), wide_values(rng, 8), wide_values(rng, 129), wide_values(rng, 20000),
          np.array([1.0, 2.0, 2.0, 2.0, 3.0]), np.array([2.0, 1.0, 2.0, 1.0]), np.array([5.0, 1.0, 1.0, 5.0, 1.0, 5.0]), np.full(9, 0.1), np.full(10, 0.1),
          rng.integers(0, 4, size=1001).astype(np.float64), rng.integers(0, 4, size=1000).astype(np.float64)]
    got = harness([["median", len(x)] + flat(x) for x in xs])
    assert np.isnan(got[0])
    for g, x in zip(got[1:], xs[1:]):
        assert g == float(np.median(x)), x[:8]


def test_norm3_adds_the_squares_in_order(harness):
    """sqrt((dx^2 + dy^2) + dz^2), nothing contracted.  (np.linalg.norm sums through a dot product, whose last bit is the BLAS's own on values as
    wide as these; on the voxel-centre distances of the crafted cases the two agree, which test_header_equals_checker_on_crafted_case holds to 1e-12.)"""
    rng = np.random.default_rng(26003)
    ab = [wide_values(rng, 6) for _ in range(50)] + [np.zeros(6), np.array([1.0, 2.0, 3.0, 1.0, 2.0, 3.0]), np.array([0.0, 4.0, 0.0, 3.0, 0.0, 0.0])]
    got = harness([["norm3"] + flat(x) for x in ab])
    for g, x in zip(got, ab):
        d = x[:3] - x[3:]
        assert g == float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    assert got[-1] == 5.0 and got[-2] == 0.0


# ---- both steps end to end against the checker ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crafted():
    from oracle import oracle as ora
    spec, header, grid, entries = cases.crafted()
    return header, grid, entries, ora.Oracle(header, grid)


CRAFTED = ["equidistant", "cutoff", "threshold", "corner", "chain", "ordinals", "aliases", "no_pairs", "nothing", "empty"]


@pytest.mark.parametrize("name", CRAFTED)
def test_header_equals_checker_on_crafted_case(harness, crafted, name):
    header, grid, entries, oracle = crafted
    e = entries[name]
    clouds = checker.atom_clouds(oracle, e["xyz"], e["radius"], e["cutoff"])
    t, p, f, got = decide(harness, header, grid, clouds, e)
    checker.assert_same_tables(got, want_of(header, grid, clouds, e), exact=True, what=name)
    n_clouds = np.array([len(c) for c in clouds], dtype=np.int64)
    if name == "ordinals":          # an atom without a cloud: no row, no pool entry, its residue no group
        assert n_clouds[3] == 0 and 3 not in p["atom_idx"] and 5 not in p["group_res"] and list(p["group_res"]) == [3, 7, 12]
    if name == "cutoff":            # several clouds, the nearest beyond the cut-off: dropped; the nearest inside: kept
        assert list(n_clouds[6:]) == [2, 2] and list(p["atom_idx"]) == [0, 1, 2, 3, 4, 5, 6]
    if name == "aliases":           # alias chains inside one residue (atoms 0, 1) and across two (3, 4 and 5, 6)
        assert list(e["alias"]) == [1, 1, 2, 4, 4, 6, 6] and list(e["residue"]) == [0, 0, 0, 1, 2, 3, 4]
        assert list(p["pool_cloud"][:2]) == [1, 1] and list(p["pool_atom"][:2]) == [0, 1]          # both atoms pool the cloud of the later one
    if name == "no_pairs":
        assert len(e["owner_key"]) == 0 and len(p["pair_a"]) == 0 and len(p["owner_state"]) == 0 and len(got["res"]["n"]) == 2
    if name == "nothing":
        assert f is None and len(t["n"]) == 0 and np.isnan(p["cutoff"][0]) and not p["owner_state"].any()
    if name == "empty":             # n == 0 with n_keys == 0: the pooling step on no atom at all
        assert f is None and len(e["xyz"]) == 0 and len(e["bonded_off"]) == 1 and list(p["first"]) == [0] and np.isnan(p["cutoff"][0])


@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("name", batch_limit_cases.WORLDS)
def test_header_equals_checker_on_worlds(harness, name, kind):
    from oracle import oracle as ora
    spec, header, grid, e = cases.world_entry(name, kind)
    clouds = checker.atom_clouds(ora.Oracle(header, grid), e["xyz"], e["radius"], e["cutoff"])
    t, p, f, got = decide(harness, header, grid, clouds, e)
    checker.assert_same_tables(got, want_of(header, grid, clouds, e), what="%s %s" % (name, kind))
    assert len(got["atom"]) >= 200 and len(p["pair_a"]) >= 100 and all(np.count_nonzero(got["owner_state"] == s) >= 3 for s in (0, 1, 2))


@pytest.mark.parametrize("name", ["orth", "alias"])
def test_header_equals_checker_on_golden_inputs(harness, name):
    from pdb_eda_amd import ccp4, synthetic, densityAnalysis
    from oracle import cpu_entry
    z, spec, st, pdb, params = load_analysis_case(name)
    header = ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(spec))
    densityAnalysis.setGlobals(params)
    host = cpu_entry.HostDensity(header, z["dens"])
    inp = densityAnalysis.DensityAnalysis(name, host, None, st, None)._cloudInputs()
    e = {k: inp[k] for k in cases.ARGS if k != "weight"}
    e.update(weight=inp["electrons"] * inp["occupancy"], cutoff=host.densityCutoff, min_electrons=25.0)
    clouds = checker.atom_clouds(host._map, e["xyz"], e["radius"], e["cutoff"])
    t, p, f, got = decide(harness, header, host._map.density, clouds, e)
    assert len(got["atom"]) >= 20 and len(got["res"]["n"]) >= 1
    assert name != "alias" or np.any(e["alias"] != np.arange(len(e["alias"])))
    checker.assert_same_tables(got, want_of(header, host._map.density, clouds, e), what=name)


# ---- edges --------------------------------------------------------------------------------------------------------------------------
def test_one_cloud_beyond_the_cutoff_is_kept_and_several_are_dropped(harness):
    """A table made by hand: twelve atoms on their cloud's centroid, atom 12 with ONE cloud 4 A away (kept: the cut-off is asked of atoms with
    several clouds only), atom 13 with two clouds 4 and 5 A away (dropped), atom 14 with two clouds 5 and 0.5 A away (kept, the nearer one its best)."""
    n = 15
    xyz = np.zeros((n, 3))
    xyz[:, 0] = 10.0 * np.arange(n)
    e = cases.chain_entry(xyz, np.full(n, 1.0), np.arange(n) + 6.0, np.arange(n) // 3, 0.5)
    group = np.array(list(range(13)) + [13, 13, 14, 14], dtype=np.int32)
    cen = xyz[group].copy()
    cen[:, 1] = [0.0] * 12 + [4.0, 4.0, 5.0, 5.0, 0.5]
    t = {"n": np.arange(len(group), dtype=np.int64) + 2, "total": np.arange(len(group)) + 1.5, "centroid": cen, "group": group}
    p, = harness([atoms_record(e), clouds_record(t), ["pool"]])
    own = np.array([0.0] * 12 + [4.0, 4.0, 0.5])
    cut = float(np.median(own) + 2.5 * np.std(own))
    assert p["rc"] == OK and p["cutoff"][0] == cut and 0.5 < cut < 4.0
    check_pool_integers(e, t, p)
    assert list(p["atom_idx"]) == list(range(13)) + [14] and list(p["pool_cloud"]) == list(range(13)) + [15, 16]
    assert list(p["atom_dist"]) == [0.0] * 12 + [4.0, 0.5] and list(p["atom_nvox"][-2:]) == [14, 18] and list(p["atom_total"][-2:]) == [13.5, 17.5]
    assert list(p["owner_state"]) == [1] * 13 + [0, 1] and list(p["group_res"]) == [0, 1, 2, 3, 4] and list(p["pool_group"][-4:]) == [3, 4, 4, 4]
    # bonds i +- 1, i +- 2 inside a residue, between pooled names: every residue whole, the last without the dropped atom 13
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b and a // 3 == b // 3 and 13 not in (a, b)]
    assert sorted(zip(p["pair_a"], p["pair_b"])) == pairs and np.array_equal(p["pair_owner"], p["pair_a"])


def test_bonded_key_out_of_range(harness, crafted):
    """Refused under a pooled owner; accepted, with the same tables, under an owner that is not pooled: only the lists of pooled owners are read."""
    header, grid, entries, oracle = crafted
    bad = cases.refusals(entries["chain"])["bonded key out of range"]
    clouds = checker.atom_clouds(oracle, bad["xyz"], bad["radius"], bad["cutoff"])
    p, = harness([atoms_record(bad), clouds_record(clouds_table(clouds)), ["pool"]])
    assert p["rc"] == BONDED_KEY_RANGE
    e = entries["ordinals"]
    n_keys = len(e["bonded_off"]) - 1
    clouds = checker.atom_clouds(oracle, e["xyz"], e["radius"], e["cutoff"])
    assert not clouds[3] and e["key"][3] == 2 and e["bonded_off"][2] == e["bonded_off"][3]          # key 2: one atom, no cloud, no bonds
    off = e["bonded_off"].copy()
    off[3:] += 1
    for k2 in (n_keys, -1):
        twisted = dict(e, bonded_off=off, bonded=np.insert(e["bonded"], e["bonded_off"][2], k2).astype(np.int32))
        t, p, f, got = decide(harness, header, grid, clouds, twisted)
        checker.assert_same_tables(got, want_of(header, grid, clouds, e), exact=True)


def test_component_rank_out_of_range(harness, crafted):
    header, grid, entries, oracle = crafted
    e = entries["chain"]
    clouds = checker.atom_clouds(oracle, e["xyz"], e["radius"], e["cutoff"])
    t, p, f, got = decide(harness, header, grid, clouds, e)
    head = [atoms_record(e), clouds_record(t), ["pool"]]
    u = checker.union_job(header, grid, clouds, p["pool_cloud"], p["pool_group"], len(p["group_res"]) + 1, p["pair_a"], p["pair_b"])
    nu = len(u[0])
    for where, value, rc in ((0, -1, COMPONENT_RANGE), (len(u[4]) - 1, nu, COMPONENT_RANGE), (len(u[4]) - 1, nu - 1, OK)):
        comp = u[4].copy()
        comp[where] = value
        assert harness(head + [finish_record(u[:4] + (comp,) + u[5:], e["min_electrons"])])[1]["rc"] == rc, (where, value)
