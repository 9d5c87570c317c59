"""Crystal contacts without a GPU: the candidate images are complete, the numpy restatement the GPU tests check against reproduces
the reference's findCoordContacts (tests/golden/contacts_ref.npz) bit for bit, and ``rows`` -> ``dumps`` gives the reference's
layout (crystalContacts.py:58-84)."""
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import contacts_checker as chk

GROUPS = ["P1", "P212121", "C2", "P61"]


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cutoff", [3.5, 5.0, 8.0])
def test_candidate_images_are_complete(group, cutoff):
    from pdb_eda_amd import crystalContacts
    rot, ortho, poly = chk.crystal(group, n_atoms=1200, seed=7)
    assert poly.min() < -1.0        # (the chain reaches outside the cell)
    cand = crystalContacts.candidateImages(rot, ortho, poly, cutoff)
    assert cand.dtype == np.int32 and cand.shape[1] == 4
    got = {tuple(int(v) for v in k) for k in cand}
    assert (0, 0, 0, 0) not in got
    assert len(got) == len(cand)
    assert [tuple(k) for k in cand.tolist()] == sorted(tuple(k) for k in cand.tolist())      # (op, n) order
    brute = np.array([(op,) + n for op in range(len(rot)) for n in itertools.product(range(-5, 6), repeat=3) if (op, n) != (0, (0, 0, 0))], dtype=np.int32)
    keep = chk.kept_images(rot, ortho, poly, brute, cutoff)
    assert keep.any()
    missing = [tuple(k) for k in brute[keep].tolist() if tuple(k) not in got]
    assert not missing, missing


def test_smtry_operators_are_printed_like_pdb_files():
    rot, ortho, _ = chk.crystal("P61")
    assert len(rot) == 6
    for m in rot:
        assert np.all(np.round(m[:, :3], 6) == m[:, :3])
    assert not np.allclose(rot[1][:, :3], np.round(rot[1][:, :3]))    # (irrational entries: cos 60 deg in Cartesian)


@pytest.mark.parametrize("case", ["random", "boundary", "duplicates"])
def test_checker_reproduces_reference_golden(case):
    z = np.load(os.path.join(GOLDEN, "contacts_ref.npz"))
    idx, dist = chk.coord_contacts(z[case + "_q"], z[case + "_p"], float(z["cutoff"]))
    assert np.array_equal(idx, z[case + "_index"])
    assert np.array_equal(dist, z[case + "_distance"])
    kidx, kdist = chk.coord_contacts(z[case + "_q"], z[case + "_p"], float(z["cutoff"]), kd=True)
    assert np.array_equal(kidx, idx) and np.array_equal(kdist, dist)
    if case == "boundary":
        assert np.count_nonzero(dist == 5.0) >= 30       # exact-boundary pairs are reported


def test_image_arithmetic_uses_the_fma_of_matvec3():
    rot, ortho, poly = chk.crystal("P61", n_atoms=20)
    ot = chk.ortho_times(ortho, (1, -1, 1))
    plain = np.asarray(ortho).dot([1.0, -1.0, 1.0])
    assert np.allclose(ot, plain, rtol=0, atol=1e-12)
    img = chk.image(rot, ortho, (0, 1, -1, 1), poly)
    assert np.array_equal(img, poly + ot)


class _Res(object):
    def __init__(self, chain, number, name):
        self.parent, self.id, self.resname = chain, (" ", number, " "), name


class _Node(object):
    def __init__(self, id_, parent=None):
        self.id, self.parent = id_, parent


class _Atom(object):
    def __init__(self, res, name, occ, coord, symmetry=None):
        self.parent, self.name, self._occ = res, name, occ
        self.coord = np.asarray(coord, dtype=np.float32)
        if symmetry is not None:
            self.symmetry = symmetry

    def get_occupancy(self):
        return self._occ


def _reference_text(headerList, result, fmt):
    """crystalContacts.py:79-84: print(...) of the CSV rows or of json.dumps."""
    if fmt == "csv":
        return "\n".join(",".join(map(str, row)) for row in [headerList] + result) + "\n"
    return json.dumps([dict(zip(headerList, row)) for row in result], indent=2, sort_keys=True) + "\n"


@pytest.mark.parametrize("fmt", ["json", "csv"])
@pytest.mark.parametrize("pdbid", [False, True])
@pytest.mark.parametrize("symmetry", [False, True])
def test_rows_and_dumps_match_reference_layout(monkeypatch, fmt, pdbid, symmetry):
    from pdb_eda_amd import crystalContacts, singleStructure
    chain = _Node("A", _Node(0))
    atoms = [_Atom(_Res(chain, 1, "ALA"), "CA", 1.0, [1.25, -2.5, 3.125], (1, 0, -1, 2) if symmetry else None),
             _Atom(_Res(chain, 2, "GLY"), "N", 0.5, [10.0, 0.1, 7.7], (0, 0, 0, 0) if symmetry else None),
             _Atom(_Res(chain, 17, "HOH"), "O", 1.0, [-3.3, 4.4, -5.5], (0, 1, 0, 1) if symmetry else None)]
    found = [(0, 4.999999999999999), (2, 5.0)]
    monkeypatch.setattr(crystalContacts, "contacts", lambda analyzer, distance=5.0, symmetryAtoms=False: (atoms, found))

    class An(object):
        pdbid = "1abc"
    header, result = crystalContacts.rows(An(), 5.0, symmetryAtoms=symmetry, includePdbid=pdbid)
    want_header = ['model', 'chain', 'residue_number', 'residue_name', "atom_name", "occupancy", "symmetry", "xyz", "crystal_contact_distance"]
    want = [[0, "A", 1, "ALA", "CA", 1.0, [1, 0, -1, 2] if symmetry else [0, 0, 0, 0], [1.25, -2.5, 3.125], 4.999999999999999],
            [0, "A", 17, "HOH", "O", 1.0, [0, 1, 0, 1] if symmetry else [0, 0, 0, 0], [float(np.float32(v)) for v in (-3.3, 4.4, -5.5)], 5.0]]
    if pdbid:
        want_header = ["pdbid"] + want_header
        want = [["1abc"] + r for r in want]
    assert header == want_header and result == want
    assert singleStructure.dumps(header, result, fmt) == _reference_text(want_header, want, fmt)
