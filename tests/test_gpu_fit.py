"""Fragment fitting on the MI355X path: a recovery test with no tuned number.

The synthetic case: on a blank 32^3 map of 0.5 A a 6-atom asymmetric fragment is placed with its pivot on a voxel centre under a known rotation;
the map is the device's own ``modelDensity`` of the placed atoms.  With the true rotation listed at a known index of a 257-entry lattice and the
27 voxels around the truth as centres, the truth must be rank 0 of its centre and the best pose of all.  ``searchFragment`` started from the
lattice WITHOUT the true rotation must never lose score from level to level and must end nearer to the truth (placed-atom RMSD) than the
lattice pass's winner; both RMSDs are printed, neither is held to a number.

The analysis layer: a synthetic entry of eight well-separated residues, one of them left out of the structure, its density the Fo-Fc map:
``fitFragment`` must put the fragment back with every atom in positive density (low == 0), and the "fit" mode must produce its table."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_kept = {}
TRUE_INDEX = 100
# an asymmetric fragment: a bent chain with a branch, bonds of about 1.5 A, different elements
FRAG = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.2, 1.3, 0.0], [3.7, 1.4, 0.3], [2.0, 2.2, 1.2], [-0.7, -1.2, 0.6]])
Z = np.array([6.0, 7.0, 6.0, 8.0, 16.0, 8.0])


def rmsd(a, b):
    return float(np.sqrt(((np.asarray(a) - np.asarray(b)) ** 2).sum(axis=1).mean()))


def synthetic_case(gpu_ctx):
    from pdb_eda_amd import ccp4, synthetic
    if "case" not in _kept:
        spec = synthetic.MapSpec(ncrs=(32, 32, 32), spacing=0.5)
        blank = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((32, 32, 32), dtype=np.float32))), "fit", ctx=gpu_ctx)
        frame = ccp4.fragmentFrame(FRAG, Z)
        true_rot = ccp4.rotationsNear(np.eye(3), 2.0, 12)[7]                                   # some rotation that no lattice holds
        centre = np.array(blank.header.crs2xyzCoord([15, 16, 14]), dtype=np.float64)
        truth = ccp4.placeFragment(frame, centre, true_rot)
        amp, expo, b_eff = ccp4.gaussianAtomTerms(Z, np.full(len(Z), 20.0), np.ones(len(Z)))
        observed = blank.modelDensity(truth, amp, expo, ccp4.modelRadii(b_eff))
        around = np.array([blank.header.crs2xyzCoord([15 + dc, 16 + dr, 14 + ds]) for ds in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)], dtype=np.float64)
        _kept["case"] = (observed, frame, true_rot, centre, truth, around)
    return _kept["case"]


def test_the_true_pose_wins_its_centre_and_all_centres(gpu_ctx):
    from pdb_eda_amd import ccp4
    observed, frame, true_rot, centre, truth, around = synthetic_case(gpu_ctx)
    rot = ccp4.rotationLattice(257)
    rot[TRUE_INDEX] = true_rot
    got = observed.poseScores(frame["xyz"], frame["weights"], rot, around, topK=3, full=True)
    at = int(np.nonzero((around == centre).all(axis=1))[0][0])
    assert at == 13 and got["bestRot"][at, 0] == TRUE_INDEX
    best_centre = int(np.argmax(got["bestScore"][:, 0]))
    print("truth scores %.6g; runner-up of its centre %.6g; best of the other centres %.6g"
          % (got["bestScore"][at, 0], got["bestScore"][at, 1], np.delete(got["bestScore"][:, 0], at).max()))
    assert best_centre == at and got["bestScore"][at, 0] == got["scores"].max()
    assert got["bestScore"][at, 0] > np.delete(got["bestScore"][:, 0], at).max()
    assert ccp4.placeFragment(frame, around[at], rot[TRUE_INDEX]).tobytes() == truth.tobytes()


def test_search_from_a_lattice_without_the_truth_ends_nearer_to_it(gpu_ctx):
    from pdb_eda_amd import ccp4
    observed, frame, true_rot, centre, truth, around = synthetic_case(gpu_ctx)
    rot = ccp4.rotationLattice(257)
    assert ccp4.rotationAngle(rot, true_rot).min() > 0.05                                       # the lattice does not hold the truth
    lattice = observed.searchFragment(frame["xyz"], frame["weights"], around, rotations=rot, nBest=3, levels=0)
    refined = observed.searchFragment(frame["xyz"], frame["weights"], around, rotations=rot, nBest=3, levels=5)
    first, last = lattice[0], refined[0]
    before, after = rmsd(first["xyz"], truth), rmsd(last["xyz"], truth)
    print("lattice pass: score %.6g, RMSD %.4f A; after %d levels: score %.6g, RMSD %.4f A (the truth scores %.6g)"
          % (first["score"], before, len(last["trace"]) - 1, last["score"], after,
             observed.poseScores(frame["xyz"], frame["weights"], true_rot[None], centre[None])["bestScore"][0, 0]))
    for pose in refined:
        assert len(pose["trace"]) == 6 and np.all(np.diff(pose["trace"]) >= 0) and pose["trace"][-1] == pose["score"]
    assert max(p["trace"][0] for p in refined) == first["score"] and last["score"] >= first["score"]
    assert after < before
    again = observed.searchFragment(frame["xyz"], frame["weights"], around, rotations=rot, nBest=3, levels=5)
    assert again[0]["xyz"].tobytes() == last["xyz"].tobytes() and again[0]["score"] == last["score"]


# ---- the analysis layer: an entry with one residue left out ---------------------------------------------------------------------------------
TEMPLATE = np.array([[-1.20, 0.35, -0.60], [0.0, 0.0, 0.0], [0.95, 1.15, 0.30], [0.75, 2.05, 1.10], [0.60, -1.25, 0.65]])      # N, CA, C, O, CB
NAMES, ELEMENTS = ["N", "CA", "C", "O", "CB"], ["N", "C", "C", "O", "C"]
OMITTED = 5


def entry(gpu_ctx):
    """Eight ALA residues 9 A apart in a P1 cell of 24 A (48^3 voxels), each under a rotation of its own; residue OMITTED is not in the structure.  The
    2Fo-Fc map is the density of all eight, the Fo-Fc map the density of the omitted one."""
    from pdb_eda_amd import ccp4, densityAnalysis, structure, synthetic
    if "entry" not in _kept:
        params = synthetic.synthetic_params()
        densityAnalysis.setGlobals(params)
        spec = synthetic.MapSpec(ncrs=(48, 48, 48), spacing=0.5)
        blank = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((48, 48, 48), dtype=np.float32))), "fit", ctx=gpu_ctx)
        rots = ccp4.rotationLattice(8)
        centres = np.array([[6.0 + 9.0 * i, 6.0 + 9.0 * j, 6.0 + 9.0 * k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]) + 0.13
        coords = [ccp4.placeFragment(TEMPLATE, centres[r], rots[r]) for r in range(8)]
        st = structure.Structure("synth")
        chain = structure.Chain("A", structure.Model(0, st))
        apart = structure.Chain("B", structure.Model(0, structure.Structure("apart")))
        serial, left_out = 0, None
        for r in range(8):
            res = structure.Residue((" ", r + 1, " "), "ALA", apart if r == OMITTED else chain)
            left_out = res if r == OMITTED else left_out
            for name, element, xyz in zip(NAMES, ELEMENTS, coords[r]):
                serial += 1
                structure.Atom(name, xyz, 1.0, 20.0, element, res, serial)
        st.header = {"resolution": 2.0}
        pdb = structure.PDBEntry(structure.PDBHeader(pdbid="fit", resolution=2.0, spaceGroup="P_1", rotationMats=[np.hstack([np.eye(3), np.zeros((3, 1))])]))
        z = np.array([params["full_atom_name_map_electrons"]["ALA_" + n] for n in NAMES], dtype=np.float64)
        amp, expo, b_eff = ccp4.gaussianAtomTerms(np.tile(z, 8), np.full(40, 20.0), np.ones(40))
        radii = ccp4.modelRadii(b_eff)
        every = blank.modelDensity(np.concatenate(coords), amp, expo, radii).density
        one = blank.modelDensity(coords[OMITTED], amp[:5], expo[:5], radii[:5]).density
        dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.asarray(every, dtype=np.float32))), "fit", ctx=gpu_ctx)
        diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.asarray(one, dtype=np.float32))), "fit", ctx=gpu_ctx)
        densityAnalysis._attachCutoffs(dens, diff)
        _kept["entry"] = (densityAnalysis.DensityAnalysis("fit", dens, diff, st, pdb), params, left_out, coords[OMITTED])
    densityAnalysis.setGlobals(_kept["entry"][1])
    return _kept["entry"]


def test_fit_fragment_puts_an_omitted_residue_back(gpu_ctx):
    from pdb_eda_amd import densityAnalysis
    an, _, left_out, truth = entry(gpu_ctx)
    fragment = densityAnalysis.fragmentFromResidue(left_out)
    assert fragment["names"] == NAMES and len(fragment["xyz"]) == 5 and np.all(fragment["electrons"] > 0)
    assert len(an.greenBlobList) >= 1
    print("green blobs: %s voxels" % [int(b.numVoxels) for b in an.greenBlobList])
    rows = an.fitFragment(fragment, topK=3)
    assert 1 <= len(rows) <= 3 and [row[0] for row in rows] == list(range(len(rows)))
    rank, centre, rotation, score, low, rscc, xyz = rows[0]
    print("best pose: score %.6g, low atoms %d, RSCC %s, RMSD to the omitted residue %.3f A" % (score, low, rscc, rmsd(xyz, truth)))
    assert low == 0 and score > 0 and len(rotation) == 9 and len(xyz) == 5
    assert all(rows[k][3] >= rows[k + 1][3] for k in range(len(rows) - 1))
    assert rscc is not None and rscc > 0
    assert np.abs(np.array(centre) - truth.mean(axis=0)).max() < 3.0                           # (inside the blob of the omitted residue, not at another residue)
    per_blob = an.calculateBlobFits(fragment)
    assert len(per_blob) >= 1 and all(len(row) == len(an.blobFitHeader) for row in per_blob)


def test_fit_mode_produces_its_table(gpu_ctx):
    from pdb_eda_amd import singleStructure
    an, _, _, _ = entry(gpu_ctx)
    assert "fit" in singleStructure.MODES
    header, rows = singleStructure.rows(an, "fit", "blob", type="ALA")
    assert header == an.blobFitHeader and len(rows) >= 1 and all(len(row) == len(header) for row in rows)
    assert rows[0][header.index("low_atoms")] == 0 and rows[0][header.index("rank")] == 0
    assert singleStructure.dumps(header, rows) and singleStructure.dumps(*singleStructure.rows(an, "fit", "blob", includePdbid=True))
    with pytest.raises(ValueError):
        singleStructure.rows(an, "fit", "atom")
