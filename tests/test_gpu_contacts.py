"""Crystal contacts on the device (pdb_eda_amd.crystalContacts, pdbeda_coord_contacts / pdbeda_crystal_contacts / pdbeda_image_coords)
against the reference's findCoordContacts (tests/golden/contacts_ref.npz) and the numpy restatement (tests/contacts_checker.py):
the same kept images, the same rows, bit-equal distances."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN
import contacts_checker as chk

pytestmark = pytest.mark.gpu

GROUPS = ["P1", "P212121", "C2", "P61"]


@pytest.mark.parametrize("case", ["random", "boundary", "duplicates"])
def test_find_coord_contacts_equals_reference(gpu_ctx, case):
    from pdb_eda_amd import crystalContacts
    z = np.load(os.path.join(GOLDEN, "contacts_ref.npz"))
    got = crystalContacts.findCoordContacts(z[case + "_q"], z[case + "_p"], float(z["cutoff"]), ctx=gpu_ctx)
    assert [i for i, _ in got] == z[case + "_index"].tolist()
    assert np.array_equal(np.array([d for _, d in got]), z[case + "_distance"])
    if case == "boundary":
        assert sum(1 for _, d in got if d == 5.0) >= 30


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cutoff", [3.5, 5.0, 8.0])
def test_crystal_contacts_match_checker(gpu_ctx, group, cutoff):
    from pdb_eda_amd import crystalContacts
    rot, ortho, poly = chk.crystal(group, n_atoms=1200, seed=11)
    rng = np.random.default_rng(5)
    ligands = np.round(rng.uniform(-6.0, 40.0, (200, 3)), 3)        # queries that are not polymer atoms (HETATM, waters)
    query = np.concatenate([poly, ligands])
    cand = crystalContacts.candidateImages(rot, ortho, poly, cutoff)
    kept, idx, dist = gpu_ctx.crystal_contacts(query, poly, rot, ortho, cand, cutoff)
    want_keep, want_idx, want_dist = chk.crystal_contacts(query, rot, ortho, poly, cand, cutoff)
    assert want_keep.any() and len(want_idx) > 0
    assert np.array_equal(kept, want_keep)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dist, want_dist)
    # the neighbour list: the kept images' atoms in (op, n, atom) order
    n = gpu_ctx.image_coords(poly, rot, ortho, cand[kept])
    assert np.array_equal(n, chk.neighbours(rot, ortho, poly, cand[kept]))


def test_coord_contacts_match_checker_across_cutoffs(gpu_ctx):
    rng = np.random.default_rng(3)
    q = rng.uniform(-20, 20, (3000, 3))
    p = rng.uniform(-25, 25, (5000, 3))
    for cutoff in (0.5, 1.7, 3.5, 5.0, 8.0):
        idx, dist = gpu_ctx.coord_contacts(q, p, cutoff)
        want_idx, want_dist = chk.coord_contacts(q, p, cutoff)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist), cutoff


@pytest.mark.parametrize("group", GROUPS)
def test_images_with_small_shifts_equal_symmetry_atoms(gpu_ctx, group):
    """For |n| <= 1 an image coordinate is the matching symmetry-atom coordinate (pdbeda_symmetry_atoms, which symmetryAtomCoords holds)."""
    rot, ortho, poly = chk.crystal(group, n_atoms=150, seed=2)
    big = 1e6
    idx, sym, xyz = gpu_ctx.symmetry_atoms(poly, rot, ortho, np.full(3, -big), np.full(3, big))
    assert len(idx) == 27 * len(rot) * len(poly)
    cand = np.array([(s[3], s[0], s[1], s[2]) for s in sym[::len(poly)]], dtype=np.int32)
    ident = np.all(cand == 0, axis=1)
    got = gpu_ctx.image_coords(poly, rot, ortho, cand[~ident]).reshape(-1, len(poly), 3)
    want = xyz.reshape(-1, len(poly), 3)[~ident]
    assert np.array_equal(got, want)


def test_large_cell_keeps_no_image(gpu_ctx):
    from pdb_eda_amd import crystalContacts
    rot, _, poly = chk.crystal("P1", n_atoms=500, seed=4)
    ortho = chk.ortho_matrix((400.0, 420.0, 450.0), (90.0, 90.0, 90.0))
    cand = crystalContacts.candidateImages(rot, ortho, poly, 5.0)
    assert len(cand) > 0
    kept, idx, dist = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    assert not kept.any() and len(idx) == 0 and len(dist) == 0


def test_bad_input_is_refused_before_any_launch(gpu_ctx):
    from pdb_eda_amd import _native
    rot, ortho, poly = chk.crystal("P212121", n_atoms=50, seed=1)
    cand = np.array([[1, 0, 0, 0]], dtype=np.int32)
    bad = poly.copy()
    bad[3, 1] = np.nan
    for args in [(poly, bad, 5.0), (bad, poly, 5.0), (poly, poly, 0.0), (poly, poly, -1.0), (poly, poly, np.inf)]:
        with pytest.raises(_native.PdbedaError) as e:
            gpu_ctx.coord_contacts(*args)
        assert e.value.code == _native.PDBEDA_ERR_ARGUMENT
    for c in ([[0, 0, 0, 0]], [[4, 0, 0, 0]], [[-1, 1, 0, 0]]):
        with pytest.raises(_native.PdbedaError):
            gpu_ctx.crystal_contacts(poly, poly, rot, ortho, np.array(c, dtype=np.int32), 5.0)
    with pytest.raises(_native.PdbedaError):
        gpu_ctx.crystal_contacts(poly, bad, rot, ortho, cand, 5.0)
    # the context still works
    idx, dist = gpu_ctx.coord_contacts(poly, poly + 0.5, 5.0)
    assert len(idx) == len(poly)


def test_two_calls_are_bit_identical(gpu_ctx):
    from pdb_eda_amd import crystalContacts
    rot, ortho, poly = chk.crystal("P61", n_atoms=3000, seed=9)
    cand = crystalContacts.candidateImages(rot, ortho, poly, 5.0)
    a = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    b = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_scale_50k_atoms_p212121(gpu_ctx):
    """A 50 000-atom P 21 21 21 entry: every atom of a dense box, ligands and waters beside it."""
    from pdb_eda_amd import crystalContacts
    cell = (120.0, 128.0, 136.0)
    ortho = chk.ortho_matrix(cell, (90.0, 90.0, 90.0))
    rot = chk.smtry("P212121", ortho)
    poly = chk.blob(50000, 21, np.array([-3.0, -3.0, -3.0]), np.array([62.0, 70.0, 74.0]))
    cand = crystalContacts.candidateImages(rot, ortho, poly, 5.0)
    kept, idx, dist = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    want_keep = chk.kept_images(rot, ortho, poly, cand, 5.0)
    assert np.array_equal(kept, want_keep) and kept.any()
    n = chk.neighbours(rot, ortho, poly, cand[kept])
    want_idx, want_dist = chk.coord_contacts(poly, n, 5.0, kd=True)
    assert len(want_idx) > 1000
    assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)


# ---- end to end: files on disk -> densityAnalysis.fromFile -> rows -> dumps ------------------------------------------------------------------
def _write_entry(tmp_path, group, n_atoms, seed):
    from pdb_eda_amd import synthetic
    cell, angles = chk.CELLS[group]
    rot, ortho, poly = chk.crystal(group, n_atoms=n_atoms, seed=seed)
    spec = synthetic.MapSpec(ncrs=(36, 40, 44), cell=cell, angles=angles)
    grid = synthetic.noise_grid(spec, seed=seed, sigma_voxels=1.5)
    for name in ("e2e.ccp4", "e2e_diff.ccp4"):
        with open(str(tmp_path / name), "wb") as fh:
            fh.write(synthetic.ccp4_bytes(spec, grid))
    lines = ["HEADER    SYNTHETIC                               01-JAN-00   7XYZ", "REMARK   2 RESOLUTION.    2.00 ANGSTROMS."]
    for k, m in enumerate(rot):
        for row in range(3):
            lines.append("REMARK 290   SMTRY%d %3d%10.6f%10.6f%10.6f%15.5f" % (row + 1, k + 1, m[row][0], m[row][1], m[row][2], m[row][3]))
    # ligands (HETATM: not polymer) and waters, half of them 1.2 A from an atom of a neighbour copy, half anywhere in the chain's box
    from pdb_eda_amd import crystalContacts
    cand = crystalContacts.candidateImages(rot, ortho, poly, 5.0)
    neigh = chk.neighbours(rot, ortho, poly, cand[chk.kept_images(rot, ortho, poly, cand, 5.0)])
    rng = np.random.default_rng(seed + 1)
    near = neigh[rng.choice(len(neigh), 15, replace=False)] + 0.7
    others = np.concatenate([near, rng.uniform(-4.0, 30.0, (15, 3))])
    serial = 0
    names = ["N", "CA", "C", "O", "CB"]
    for i, xyz in enumerate(poly):
        serial += 1
        res = i // 5 + 1
        lines.append("ATOM  %5d  %-3s ALA A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f           %s" % (serial, names[i % 5], res, xyz[0], xyz[1], xyz[2], 1.0, 20.0, names[i % 5][0]))
    for k, xyz in enumerate(np.round(others, 3)):
        serial += 1
        resname, name = ("HOH", "O") if k % 2 else ("LIG", "C1")
        lines.append("HETATM%5d  %-3s %s B%4d    %8.3f%8.3f%8.3f%6.2f%6.2f           %s" % (serial, name, resname, 500 + k, xyz[0], xyz[1], xyz[2], 0.5, 30.0, name[0]))
    lines.append("END")
    with gzip.open(str(tmp_path / "pdb7xyz.ent.gz"), "wt") as fh:
        fh.write("\n".join(lines) + "\n")
    return rot


def _checker_rows(an, distance, symmetryAtoms, includePdbid):
    from pdb_eda_amd import crystalContacts
    poly = crystalContacts.polymerCoordinates(an)
    rot = np.array([np.asarray(m, dtype=np.float64) for m in an.pdbObj.header.rotationMats])
    ortho = np.asarray(an.densityObj.header.orthoMat, dtype=np.float64)
    cand = crystalContacts.candidateImages(rot, ortho, poly, distance)
    if symmetryAtoms:
        atoms, query = an.symmetryAtoms, np.asarray(an.symmetryAtomCoords, dtype=np.float64)
    else:
        atoms = list(an.biopdbObj.get_atoms())
        query = np.asarray([a.coord for a in atoms], dtype=np.float64)
    _, idx, dist = chk.crystal_contacts(query, rot, ortho, poly, cand, distance)
    header = list(crystalContacts.headerList)
    result = []
    for index, d in zip(idx.tolist(), dist.tolist()):
        atom = atoms[index]
        result.append([atom.parent.parent.parent.id, atom.parent.parent.id, atom.parent.id[1], atom.parent.resname, atom.name, atom.get_occupancy(),
                       [x for x in atom.symmetry] if symmetryAtoms else [0, 0, 0, 0], [float(c) for c in atom.coord], d])
    if includePdbid:
        header = ["pdbid"] + header
        result = [[an.pdbid] + r for r in result]
    return header, result


@pytest.mark.parametrize("group", ["P212121", "C2"])
def test_end_to_end_rows_and_text(gpu_ctx, tmp_path, group):
    from pdb_eda_amd import crystalContacts, densityAnalysis, singleStructure
    _write_entry(tmp_path, group, 700, 13)
    an = densityAnalysis.fromFile(str(tmp_path / "pdb7xyz.ent.gz"), str(tmp_path / "e2e.ccp4"), str(tmp_path / "e2e_diff.ccp4"))
    assert an != 0
    assert len(crystalContacts.polymerCoordinates(an)) == 700
    for symmetryAtoms, includePdbid in ((False, False), (False, True), (True, False)):
        header, result = crystalContacts.rows(an, 5.0, symmetryAtoms=symmetryAtoms, includePdbid=includePdbid)
        want_header, want = _checker_rows(an, 5.0, symmetryAtoms, includePdbid)
        assert header == want_header
        assert len(result) > 0 and result == want
        if symmetryAtoms:
            assert any(r[-1] == 0.0 for r in result)        # symmetry atoms that coincide with a neighbour copy (the reference's quirk)
            assert any(r[-3] != [0, 0, 0, 0] for r in result)
        else:
            assert any(r[-6] in ("HOH", "LIG") for r in result)         # (residue_name)
        for fmt in ("json", "csv"):
            assert singleStructure.dumps(header, result, fmt) == singleStructure.dumps(want_header, want, fmt)
    # the neighbour list: the kept images' atoms
    n = crystalContacts.simulateCrystalNeighborCoordinates(an, 5.0)
    images, poly = crystalContacts.keptImages(an, 5.0)
    rot = np.array([np.asarray(m, dtype=np.float64) for m in an.pdbObj.header.rotationMats])
    assert n.shape == (len(images) * len(poly), 3)
    assert np.array_equal(n, chk.neighbours(rot, np.asarray(an.densityObj.header.orthoMat), poly, images))
