"""Crystal contacts without a GPU: the candidate images are complete, the numpy restatement the GPU tests check against reproduces
the reference's findCoordContacts (tests/golden/contacts_ref.npz) bit for bit, and ``rows`` -> ``dumps`` gives the reference's
layout (crystalContacts.py:58-84)."""
import itertools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import contacts_cases as cases
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

# ---- the edge cases of tests/contacts_cases.py reach the corners they are named for (the checker alone; tests/test_gpu_contacts_edges.py runs
# ---- them on the device) ----------------------------------------------------------------------------------------------------------------------


def test_large_coord_cases_leave_the_pinned_block():
    """Mixed: 300 000 index rows are 2 400 000 bytes <= 4 MiB, the distance rows behind them do not fit; 8 (n_q + n_p) > 2^22, so the grid is
    bounded by 2^22 cells and its edge coarsens.  Device: 600 000 rows are 4 800 000 bytes > 4 MiB per column."""
    q, p, cutoff = cases.coord_case("mixed")
    assert 8 * len(q) <= cases.PINNED_BLOCK < 16 * len(q) and 8 * (len(q) + len(p)) > 1 << 22
    edge, dims, n_cells, steps = cases.query_grid(q, cutoff, len(q) + len(p))
    print("mixed: edge %.10f dims %s, %d steps" % (edge, dims, steps))
    assert steps >= 1 and n_cells <= 1 << 22 and 4 * n_cells > cases.PINNED_BLOCK
    assert len(cases.expected_coord("mixed")[0]) >= 10000
    q, p, cutoff = cases.coord_case("device")
    assert 8 * len(q) > cases.PINNED_BLOCK
    assert len(cases.expected_coord("device")[0]) >= 10000
    # the KD checker is the brute one wherever both are affordable: on a slice of the queries
    for family in ("mixed", "device"):
        q, p, cutoff = cases.coord_case(family)
        idx, dist = cases.expected_coord(family)
        sl = slice(1000, 1064) if family == "mixed" else slice(0, 20000)
        bidx, bdist = chk.coord_contacts(q[sl], p, cutoff)
        m = (idx >= sl.start) & (idx < sl.stop)
        assert len(bidx) >= 3 and np.array_equal(bidx + sl.start, idx[m]) and np.array_equal(bdist, dist[m])


def test_many_candidates_keep_eight_images():
    query, poly, rot, ortho, cand, cutoff = cases.many_candidates()
    assert len(cand) == 103 ** 3 - 1 == 1092726 and 4 * len(cand) > cases.PINNED_BLOCK
    keep = chk.kept_images_diag(np.diag(ortho), poly, cand, cutoff)
    assert keep.sum() == 8
    want = {(0, 1, 0, 0), (0, 0, 1, 0), (0, 1, 1, 0), (0, 1, 1, 1)}
    assert {tuple(k) for k in cand[keep].tolist()} == want | {(0, -a, -b, -c) for _, a, b, c in want}
    pick = np.unique(np.concatenate([np.random.default_rng(1).choice(len(cand), 300, replace=False), np.nonzero(keep)[0]]))
    assert np.array_equal(chk.kept_images(rot, ortho, poly, cand[pick], cutoff), keep[pick])
    idx, dist = chk.coord_contacts(query, chk.neighbours(rot, ortho, poly, cand[keep]), cutoff)
    assert len(query) == 5 and len(idx) >= 3


def test_many_images_leave_the_pinned_block():
    poly, rot, ortho, cand = cases.many_images()
    assert len(cand) * len(poly) >= 200000 and 24 * len(cand) * len(poly) > cases.PINNED_BLOCK
    assert len({tuple(k) for k in cand.tolist()}) == len(cand) and len(set(cand[:, 0].tolist())) >= 2


def test_ordinary_cases_have_rows_and_kept_images():
    idx, _ = cases.expected_coord("ordinary")
    assert 100 <= len(idx) < len(cases.coord_case("ordinary")[0])
    keep, idx, _ = cases.expected_crystal("ordinary")
    assert keep.any() and not keep.all() and 100 <= len(idx) < len(cases.crystal_case("ordinary")[0])
    keep, idx, _ = cases.expected_crystal("far")
    assert keep.any() and len(idx) == 0


@pytest.mark.parametrize("name", sorted(cases.degenerate_coord()))
def test_degenerate_coord_cases(name):
    q, p, cutoff = cases.coord_case("degenerate", name)
    idx, dist = cases.expected_coord("degenerate", name)
    if len(q) * len(p) <= 4e7:
        kidx, kdist = chk.coord_contacts(q, p, cutoff, kd=True)
        assert np.array_equal(kidx, idx) and np.array_equal(kdist, dist)
    if name == "one on one":
        assert idx.tolist() == [0] and dist.tolist() == [0.0]
    elif name.startswith("at cutoff"):
        assert idx.tolist() == [0] and dist.tolist() == [5.0] and cutoff == 5.0
    elif name.startswith("past cutoff") or name.startswith("below cutoff"):
        assert len(idx) == 0 and cases.BELOW_FIVE <= cutoff <= 5.0
    elif name == "signed zeros":
        assert idx.tolist() == [0, 1, 2] and dist.tolist() == [0.0, 0.0, 1.0]
    elif name.startswith("collinear"):
        assert np.linalg.matrix_rank(np.concatenate([q, p]) - q[0]) == 1 and 200 <= len(idx) < len(q)
    elif name == "coplanar":
        assert np.linalg.matrix_rank(np.concatenate([q, p]) - q[0]) == 2 and 200 <= len(idx) < len(q)
    elif name == "one crowded cell":
        assert len(np.unique(cases.cell_of(q, cutoff, len(q) + len(p), p))) == 1 and len(p) == 5000 and 50 <= len(idx) < len(q)
    else:
        assert name.startswith("shifted") and min(q.min(), p.min()) > 8900.0 and 200 <= len(idx) < len(q)


@pytest.mark.parametrize("name", sorted(cases.degenerate_crystal()))
def test_degenerate_crystal_cases(name):
    query, poly, rot, ortho, cand, cutoff = cases.crystal_case("degenerate", name)
    keep, idx, dist = cases.expected_crystal("degenerate", name)
    _, dims, n_cells, _ = cases.cell_grid(poly.min(axis=0), poly.max(axis=0), cutoff, len(poly))
    print("%s: polymer grid %s, %d of %d images kept, %d rows" % (name, dims, keep.sum(), len(cand), len(idx)))
    assert (dims[0] > 1 and dims[1:] == (1, 1)) if name == "collinear atoms" else n_cells == 1
    assert keep.any() and not keep.all() and 10 <= len(idx) < len(query)
    bidx, bdist = chk.coord_contacts(query, chk.neighbours(rot, ortho, poly, cand[keep]), cutoff)
    assert np.array_equal(bidx, idx) and np.array_equal(bdist, dist)


@pytest.mark.parametrize("name", sorted(cases.grid_corners()))
def test_grid_corner_cases(name):
    q, p, cutoff = cases.coord_case("corners", name)
    idx, dist = cases.expected_coord("corners", name)
    edge, dims, n_cells, steps = cases.query_grid(q, cutoff, len(q) + len(p))
    print("%s: edge %.9g dims %s = %d cells, %d steps, %d rows" % (name, edge, dims, n_cells, steps, len(idx)))
    assert 200 <= len(idx) < len(q)
    kidx, kdist = chk.coord_contacts(q, p, cutoff, kd=True)
    assert np.array_equal(kidx, idx) and np.array_equal(kdist, dist)
    if name in cases.GRID_CORNERS:
        assert n_cells == cases.GRID_CORNERS[name][3] and steps == 0
        cell = cases.cell_of(q, cutoff, len(q) + len(p), p)
        # points in the first and the last cell of every axis; rows in the first and the last cell of every axis that a query can lie in
        c3 = np.stack([cell % dims[0], cell // dims[0] % dims[1], cell // (dims[0] * dims[1])], axis=1)
        qcell = cases.cell_of(q, cutoff, len(q) + len(p), q[idx])
        q3 = np.stack([qcell % dims[0], qcell // dims[0] % dims[1], qcell // (dims[0] * dims[1])], axis=1)
        for axis in range(3):
            assert {0, dims[axis] - 1} <= set(c3[:, axis].tolist())
            assert {2, dims[axis] - 3} <= set(q3[:, axis].tolist())
        beyond = cell[cases.nearest_point(q, p, idx)] >= cases.SCAN_TILE
        if name == "one tile":
            assert n_cells == cases.SCAN_TILE
        elif name == "one tile and eight cells":
            # The last eight cells are the far corner of the last y row of the last z layer.  The last cell of an axis begins
            # (dim - 1) * edge > extent + 3 cutoffs from the grid's origin, more than a cutoff beyond every query: no row can have its nearest
            # point there.  They hold points, which the scan's second trip counts; "one tile and eight z layers" has the rows.
            assert not beyond.any() and np.count_nonzero(cell >= cases.SCAN_TILE) >= 1
        else:
            assert np.count_nonzero(beyond) >= 20
    elif name == "lower bound of the cap":
        assert len(q) + len(p) < 512 and steps >= 1 and n_cells <= 4096
        assert cases.query_grid(q, cutoff, 1 << 30)[2] > 4096      # (what the box wants at the first edge)
    else:
        assert steps >= 20 and n_cells <= 8 * (len(q) + len(p))


def test_exact_boundary_images():
    poly, rot, ortho, cand = cases.boundary_identity()
    keep = chk.kept_images(rot, ortho, poly, cand, 5.0)
    print("identity: %d candidates" % len(cand))
    assert [tuple(k) for k in cand[keep].tolist()] == [(0, -1, 0, 0), (0, 1, 0, 0)]
    assert np.array_equal(chk.kept_images_diag(np.diag(ortho), poly[:40], cand, 5.0), chk.kept_images(rot, ortho, poly[:40], cand, 5.0))
    assert np.array_equal(chk.kept_images_diag(np.diag(ortho), poly[:2], cand, 5.0), keep)          # (the two atoms that decide)
    idx, dist = chk.coord_contacts(poly, chk.neighbours(rot, ortho, poly, cand[keep]), 5.0)
    assert idx.tolist() == [0, 1] and dist.tolist() == [5.0, 5.0]
    assert not chk.kept_images(rot, ortho, poly, cand, cases.BELOW_FIVE).any()
    poly, rot, ortho, cand = cases.boundary_twofold()
    keep = chk.kept_images(rot, ortho, poly, cand, 5.0)
    assert [tuple(k) for k in cand[keep].tolist()] == [(0, -1, 0, 0), (0, 1, 0, 0), (1, -1, 0, 0), (1, 0, 0, 0)]
    idx, dist = chk.coord_contacts(poly, chk.neighbours(rot, ortho, poly, cand[keep]), 5.0)
    assert idx.tolist() == [0, 1, 2, 3] and dist.tolist() == [5.0] * 4
    assert not chk.kept_images(rot, ortho, poly, cand, cases.BELOW_FIVE).any()


def test_largest_shift_is_far_from_the_cell():
    poly, rot, ortho, _ = cases.boundary_identity()
    cand = np.array([[0, cases.MAX_SHIFT, 0, 0]], dtype=np.int32)
    assert not chk.kept_images(rot, ortho, poly, cand, 5.0).any()
    n = chk.neighbours(rot, ortho, poly, cand)
    assert n[:, 0].min() > 4.19e7 and np.array_equal(n[:, 1:], poly[:, 1:]) and np.array_equal(n[:, 0], poly[:, 0] + 40.0 * 2 ** 20)
