"""Real-space refinement on the MI355X path: DensityMatrix.refineGaussianAtoms on a synthetic case whose truth is known, and the analysis
layer (calculateAtomGradients, refineAtoms, refineSummary, the "refine" mode) on the small golden entry.

The synthetic case: about a dozen atoms on ``wide`` (48 x 12 x 12 voxels of 0.5 A), the observed map the device's own model of the true atoms;
the coordinates are perturbed by 0.2 A rms and the B-factors by +-20 % (seeded).  Asserted: the trace of T never increases, the final T is
strictly below the first, and the rms coordinate error and the rms B error afterwards are below those before.  The values reached are
printed and recorded in DESIGN.md 4.18, not asserted.  A second run gives the same bytes."""
import io

import numpy as np
import pytest

from conftest import load_analysis_case
import gradient_cases as cases

pytestmark = pytest.mark.gpu

_kept = {}


def synthetic_case(gpu_ctx):
    """(observed DensityMatrix, the true atoms, the perturbed start), made once."""
    from pdb_eda_amd import ccp4, synthetic
    if "case" not in _kept:
        rng = np.random.default_rng(2029)
        spec = cases.spec_of("wide")
        nc, nr, ns = spec.ncrs
        blank = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((ns, nr, nc), dtype=np.float32))), "wide", ctx=gpu_ctx)
        lo, hi = cases.box_of("wide")
        n = 12
        xyz = np.stack([np.linspace(lo[0] + 2.5, hi[0] - 2.5, n), np.full(n, 0.5 * (lo[1] + hi[1])), np.full(n, 0.5 * (lo[2] + hi[2]))], axis=1)
        xyz += rng.uniform(-0.6, 0.6, size=(n, 3))                                           # a jittered chain: neighbours 1.7 A apart overlap
        z = rng.choice([6.0, 7.0, 8.0], size=n)
        b = rng.uniform(15.0, 30.0, size=n)
        occ = np.ones(n)
        amp, expo, b_eff = ccp4.gaussianAtomTerms(z, b, occ)
        observed = blank.modelDensity(xyz, amp, expo, ccp4.modelRadii(b_eff))
        start_xyz = xyz + rng.normal(0.0, 0.2 / np.sqrt(3.0), size=(n, 3))                    # 0.2 A rms in length
        start_b = b * np.where(rng.random(n) < 0.5, 0.8, 1.2)
        _kept["case"] = (observed, (xyz, z, b, occ), (start_xyz, start_b))
    return _kept["case"]


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt((a * a).sum() / len(a)))


def test_refinement_recovers_a_perturbed_model(gpu_ctx):
    observed, (xyz, z, b, occ), (start_xyz, start_b) = synthetic_case(gpu_ctx)
    out = observed.refineGaussianAtoms(start_xyz, z, start_b, occ, what=("xyz", "b"), cycles=10, maxShift=0.3)
    trace = out["trace"]
    t = np.array(trace["T"])
    before = (rms(np.linalg.norm(start_xyz - xyz, axis=1)), rms(start_b - b))
    after = (rms(np.linalg.norm(out["xyz"] - xyz, axis=1)), rms(out["bfactors"] - b))
    print("T per cycle: %s" % ", ".join("%.6g" % v for v in t))
    print("cc %.6f -> %.6f, scale %.6f -> %.6f, halvings %s" % (trace["cc"][0], trace["cc"][-1], trace["scale"][0], trace["scale"][-1], trace["halvings"]))
    print("rms coordinate error %.4f -> %.4f A, rms B error %.3f -> %.3f A^2" % (before[0], after[0], before[1], after[1]))
    assert len(t) >= 2 and np.all(np.diff(t) <= 0) and t[-1] < t[0]
    assert after[0] < before[0] and after[1] < before[1]
    assert np.array_equal(out["occupancies"], occ) and np.all(out["bfactors"] >= 10.0)
    assert len(trace["scale"]) == len(trace["cc"]) == len(t) == len(trace["halvings"]) + 1
    _kept["first"] = out


def test_a_second_run_gives_the_same_bytes(gpu_ctx):
    observed, (xyz, z, b, occ), (start_xyz, start_b) = synthetic_case(gpu_ctx)
    first = _kept.get("first") or observed.refineGaussianAtoms(start_xyz, z, start_b, occ, what=("xyz", "b"), cycles=10, maxShift=0.3)
    again = observed.refineGaussianAtoms(start_xyz, z, start_b, occ, what=("xyz", "b"), cycles=10, maxShift=0.3)
    for name in ("xyz", "bfactors", "occupancies"):
        assert again[name].tobytes() == first[name].tobytes()
    assert np.array(again["trace"]["T"]).tobytes() == np.array(first["trace"]["T"]).tobytes() and again["trace"]["halvings"] == first["trace"]["halvings"]


def test_images_fold_through_their_rotations(gpu_ctx):
    """Each true atom twice, itself and its copy under a 2-fold about z through the box centre (copies far from their originals): refined
    with ``images``, the copies follow their atoms and T falls as before."""
    from pdb_eda_amd import ccp4, synthetic
    observed, (xyz, z, b, occ), (start_xyz, start_b) = synthetic_case(gpu_ctx)
    lo, hi = cases.box_of("wide")
    centre = 0.5 * (lo + hi)
    rot = np.diag([-1.0, -1.0, 1.0])
    twofold = np.hstack([rot, (centre - rot.dot(centre))[:, None]])
    half = slice(0, 5)                                                                        # atoms of the left half; their copies land on the right
    ops = [ccp4.identityOperator(), twofold]
    amp, expo, b_eff = ccp4.gaussianAtomTerms(np.tile(z[half], 2), np.tile(b[half], 2), np.tile(occ[half], 2))
    both = np.concatenate([xyz[half], ccp4.applyOperator(twofold, xyz[half])])
    target = observed.modelDensity(both, amp, expo, ccp4.modelRadii(b_eff))
    out = target.refineGaussianAtoms(start_xyz[half], z[half], start_b[half], occ[half], what=("xyz", "b"), cycles=6, images=ops)
    t = np.array(out["trace"]["T"])
    print("with a 2-fold: T %s" % ", ".join("%.6g" % v for v in t))
    assert np.all(np.diff(t) <= 0) and t[-1] < t[0]
    assert rms(np.linalg.norm(out["xyz"] - xyz[half], axis=1)) < rms(np.linalg.norm(start_xyz[half] - xyz[half], axis=1))


# ---- the analysis layer on the small golden entry ---------------------------------------------------------------------------------------
def analysis(gpu_ctx, name="orth"):
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    if name not in _kept:
        z, spec, st, pdb, params = load_analysis_case(name)
        densityAnalysis.setGlobals(params)
        dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), name, ctx=gpu_ctx)
        diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), name, ctx=gpu_ctx)
        densityAnalysis._attachCutoffs(dens, diff)
        st.header = {"resolution": 2.0}
        _kept[name] = (densityAnalysis.DensityAnalysis(name, dens, diff, st, pdb), params)
    densityAnalysis.setGlobals(_kept[name][1])
    return _kept[name][0]


def test_atom_gradients_of_the_golden_entry(gpu_ctx):
    """One finite row per atom of the asymmetric unit; its image-folded gradient equals the sum of the per-image rows of a DIRECT atomMoments
    call on the residual, pushed through the operators on the host (a plain loop, not the library's fold)."""
    from pdb_eda_amd import ccp4, densityAnalysis as da, structure
    an = analysis(gpu_ctx)
    table = an.calculateAtomGradients()
    cols = structure.columns(an.biopdbObj)
    assert len(table) == len(cols.atoms) > 0 and all(len(row) == len(an.atomGradientHeader) for row in table)
    numbers = np.array([row[6:] for row in table], dtype=np.float64)
    assert np.all(np.isfinite(numbers)) and np.any(numbers[:, 1:6] != 0) and numbers[:, -1].max() > 0
    # the direct route
    d, model = an.densityObj, an.modelDensityObj
    fit = an.modelCorrelation()
    xyz, amp, expo, radii, _ = an._modelAtoms()
    residual = d._residual(model, fit["scale"], fit["offset"])
    got = residual.atomMoments(xyz, expo, radii, uniqueBox=True)
    atoms = an._refinementAtoms()
    rows, ops = atoms["rows"], atoms["operators"]
    assert len(rows) == len(xyz) and np.allclose(np.einsum("kij,kj->ki", ops[:, :, :3], atoms["xyz"][rows]) + ops[:, :, 3], xyz, atol=1e-9)      # the operators reproduce the symmetry atoms
    assert (np.bincount(rows) > 1).any()                                                      # (some atom has symmetry copies inside the map: the fold does something)
    each = ccp4.gaussianAtomGradients(got["moments"], atoms["electrons"][rows], atoms["bfactors"][rows], atoms["occupancies"][rows], blur=da.modelBlur)
    want, mag = np.zeros((len(cols.atoms), 5)), np.zeros((len(cols.atoms), 5))
    for k in range(len(rows)):
        at = atoms["atomRows"][rows[k]]
        want[at, 0:3] += -fit["scale"] * ops[k, :, :3].T.dot(each["dXyz"][k])
        want[at, 3] += -fit["scale"] * each["dB"][k]
        want[at, 4] += -fit["scale"] * each["dOcc"][k]
        mag[at, 0:3] += abs(fit["scale"]) * np.abs(ops[k, :, :3]).T.dot(np.abs(each["dXyz"][k]))
        mag[at, 3] += abs(fit["scale"] * each["dB"][k])
        mag[at, 4] += abs(fit["scale"] * each["dOcc"][k])
    # the same fp64 terms in another order and grouping: a copy's contribution carries four roundings (a dot product of three, the scale), the
    # sum over m copies m - 1 more, on either side: (m + 3) 2^-52 of the magnitudes
    copies = int(np.bincount(rows).max())
    assert np.all(np.abs(numbers[:, 1:6] - want) <= (copies + 3) * 2.0 ** -52 * mag)


def test_refine_mode_produces_its_two_tables(gpu_ctx):
    from pdb_eda_amd import singleStructure, structure
    an = analysis(gpu_ctx)
    n = len(structure.columns(an.biopdbObj).atoms)
    header, rows = singleStructure.rows(an, "refine", "atom")
    assert header == an.refineAtomHeader and len(rows) == n and all(len(row) == len(header) for row in rows)
    assert np.all(np.isfinite(np.array([row[6:] for row in rows], dtype=np.float64)))
    header, summary = singleStructure.rows(an, "refine", "summary")
    assert len(summary) == 1 and len(summary[0]) == len(header) and header[:4] == ["num_atoms", "cycles", "target_before", "target_after"]
    values = dict(zip(header, summary[0]))
    print("refine summary: %s" % values)
    assert values["target_after"] <= values["target_before"] and values["num_atoms"] > 0 and values["rms_shift"] >= 0
    assert singleStructure.dumps(header, summary) and singleStructure.dumps(*singleStructure.rows(an, "refine", "atom", includePdbid=True))
    with pytest.raises(ValueError):
        singleStructure.rows(an, "refine", "residue")
