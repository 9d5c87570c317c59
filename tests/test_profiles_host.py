"""The radial-profile contract without a GPU: the numpy checker (tests/profiles_checker.py, the yardstick of
tests/test_gpu_profiles.py) tied to the pinned oracle's sphere lists, the new name of the C-ABI in the built library and the
ctypes stub, the new mode and headers, and the per-atom-type median / profile-radius logic on canned shells."""
import ctypes

import numpy as np
import pytest

from conftest import load_case
import profiles_cases
import profiles_checker


@pytest.mark.parametrize("name", ["orth", "orth_sub", "hex", "tric"])
def test_checker_shells_add_up_to_the_oracle_sphere(name):
    """Shells partition the sphere of getSphereCrsFromXyz: per atom the shell counts add up to the oracle's list at cutoff 0,
    the significant counts to its list at +-1.5 sigma (positions outside the stored box and on voxel centres included)."""
    from oracle import oracle as ora
    z, header, grid = load_case(name)
    o = ora.Oracle(header, grid)
    xyz = profiles_cases.case_atoms(name, header)
    assert len(xyz) == 32
    sigma = float(z["mean"]) + 1.5 * float(z["std"])
    radius, n_shells = 1.7, 9
    plain = profiles_checker.radial_profiles(header, grid, xyz, radius, n_shells, 0.0)
    assert np.array_equal(plain["n"], plain["n_sig"]) and np.array_equal(plain["sum"], plain["sum_sig"])
    assert plain["n"].sum() > 0
    for cut in (sigma, -sigma):
        got = profiles_checker.radial_profiles(header, grid, xyz, radius, n_shells, cut)
        assert np.array_equal(got["n"], plain["n"])
        for a, p in enumerate(xyz):
            assert plain["n"][a].sum() == len(o.sphere_crs(p, radius, 0.0)), (name, a)
            assert got["n_sig"][a].sum() == len(o.sphere_crs(p, radius, cut)), (name, a, cut)
            assert bool(plain["valid"][a]) == o.valid_xyz(p, radius), (name, a)
    if name in ("orth_sub", "hex"):          # stored voxels missing from the cell: both answers occur
        assert plain["valid"].any() and not plain["valid"].all()


def test_checker_shell_rule_on_a_hand_made_grid():
    """d == 0 lies in shell 0, d == radius in the last shell, a voxel exactly on an inner boundary in the outer of the two."""
    from pdb_eda_amd import ccp4, synthetic
    ncrs = (9, 9, 9)
    header = ccp4.DensityHeader.fromFileHeader(synthetic.ccp4_header_bytes(synthetic.MapSpec(ncrs=ncrs, spacing=0.5)))
    grid = np.zeros((9, 9, 9), dtype=np.float32)
    grid[4, 4, 4] = 8.0          # the centre
    grid[4, 4, 5] = 1.0          # c + 1: d = 0.5, on the boundary of shells 0 | 1 (w = 0.5)
    grid[4, 4, 6] = 2.0          # c + 2: d = 1.0 == radius
    centre = header.crs2xyzCoord([4, 4, 4])
    got = profiles_checker.radial_profiles(header, grid, [centre], 1.0, 2, 0.0)
    assert got["n"].tolist() == [[1, 32]]                      # 33 voxels within 1.0 of a voxel centre at spacing 0.5
    assert got["sum"].tolist() == [[8.0, 3.0]]
    assert got["boundary_ties"].tolist() == [12]               # the six axial neighbours at d = w and the six at d = 2 w
    pos = profiles_checker.radial_profiles(header, grid, [centre], 1.0, 2, 1.5)
    assert pos["n_sig"].tolist() == [[1, 1]] and pos["sum_sig"].tolist() == [[8.0, 2.0]]
    neg = profiles_checker.radial_profiles(header, grid, [centre], 1.0, 2, -1.5)
    assert neg["n_sig"].tolist() == [[0, 0]] and neg["sum_sig"].tolist() == [[0.0, 0.0]]


def test_abi_has_the_entry_point():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native
    assert "pdbeda_radial_profiles" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "pdbeda_radial_profiles")
    assert hasattr(_native.DeviceMap, "radial_profiles")


def test_mode_and_headers():
    from pdb_eda_amd import ccp4, densityAnalysis as da, singleStructure
    assert "profile" in singleStructure.MODES
    assert ("profile", "atom") in singleStructure.TABLES and ("profile", "atom-type") in singleStructure.TABLES
    lead = da.DensityAnalysis.atomRegionDensityHeader[:6]
    assert da.DensityAnalysis.atomRadialProfileHeader == lead + ['atom_type', 'electrons', 'bfactor', 'valid', 'shell_voxels', 'shell_density',
                                                                 'shell_significant_voxels', 'shell_significant_density']
    assert da.DensityAnalysis.atomTypeRadialProfileHeader == ['atom_type', 'num_atoms', 'optimized_radius', 'shell_outer_radius',
                                                              'median_cumulative_density_per_electron', 'profile_radius']
    assert hasattr(ccp4.DensityMatrix, "radialProfiles")


class _CannedMap(object):
    """Stands in for the 2Fo-Fc DensityMatrix: atom i sits at (i, 0, 0) and gets row i of the canned shells."""
    meanDensity, stdDensity = 0.25, 0.5

    def __init__(self, sum_sig):
        self.sum_sig = np.asarray(sum_sig, dtype=np.float64)
        self.calls = []

    def radialProfiles(self, xyz, maxRadius, nShells, cutoff):
        self.calls.append((len(xyz), maxRadius, nShells, cutoff))
        rows = np.asarray(xyz)[:, 0].astype(np.int64)
        s = self.sum_sig[rows][:, :nShells]
        n = np.full(s.shape, 3, dtype=np.int64)
        return {"n": n, "sum": s + 1.0, "nSig": n - 1, "sumSig": s, "valid": np.ones(len(rows), dtype=bool)}


def _canned_analysis():
    from pdb_eda_amd import densityAnalysis as da, structure, synthetic
    da.setGlobals(synthetic.synthetic_params())
    st = structure.Structure("canned")
    chain = structure.Chain("A", structure.Model(0, st))
    spec = [  # (hetero flag, residue number, atom name, occupancy)
        (" ", 1, "N", 1.0), (" ", 1, "CA", 1.0), (" ", 1, "CB", 1.0), (" ", 1, "XX9", 1.0),
        (" ", 2, "N", 1.0), (" ", 2, "CA", 0.0), (" ", 2, "O", 1.0),
        (" ", 3, "N", 0.5), (" ", 3, "CA", 1.0), (" ", 3, "O", 1.0),
        ("H_LIG", 4, "N", 1.0), ("H_LIG", 4, "CA", 1.0)]
    res, last = None, None
    for i, (het, num, name, occ) in enumerate(spec):
        if (het, num) != last:
            res, last = structure.Residue((het, num, " "), "ALA", chain), (het, num)
        structure.Atom(name, np.array([float(i), 0.0, 0.0]), occ, 10.0 + i, name[0], res, i + 1)
    # cumulative sums per electron (N: 8 e, CA: 7 e, CB: 9 e, O: 8 e) against a ratio of 0.5:
    sum_sig = np.zeros((len(spec), 4))
    sum_sig[0] = [0.8, 0.8, 1.6, 0.8]        # N   cum / 8 = 0.1 0.2 0.4 0.5
    sum_sig[4] = [1.6, 1.6, 1.6, 1.6]        # N             0.2 0.4 0.6 0.8
    sum_sig[7] = [0.8, 1.6, 2.4, 3.2]        # N             0.1 0.3 0.6 1.0      median: 0.1 0.3 0.6 0.8 -> reached in shell 2
    sum_sig[1] = [0.7, 0.7, 0.7, 0.7]        # CA  cum / 7 = 0.1 0.2 0.3 0.4
    sum_sig[5] = [70.0, 70.0, 70.0, 70.0]    # CA with occupancy 0: not eligible
    sum_sig[8] = [1.4, 0.0, 0.7, 0.0]        # CA            0.2 0.2 0.3 0.3      median: 0.15 0.2 0.3 0.35 -> never
    sum_sig[2] = [4.5, 0.0, 0.0, 0.0]        # CB  cum / 9 = 0.5 ...: ONE atom, reached in shell 0
    sum_sig[6] = [0.0, 0.0, 0.0, 3.2]        # O   cum / 8 = 0 0 0 0.4
    sum_sig[9] = [0.0, 0.0, 0.0, 4.8]        # O             0 0 0 0.6            median: 0 0 0 0.5 -> reached in the last shell
    sum_sig[10] = sum_sig[11] = [90.0] * 4   # hetero residue: not eligible
    dens = _CannedMap(sum_sig)
    an = da.DensityAnalysis("canned", dens, None, st, None)
    return an, dens, spec, sum_sig


def test_atom_type_profiles_on_canned_shells():
    an, dens, spec, sum_sig = _canned_analysis()
    with pytest.raises(RuntimeError):
        an._densityElectronRatio = 0        # (no ratio: the existing error, before any device call)
        an._medians = {}
        an.atomTypeRadialProfiles(2.0, 4)
    assert dens.calls == []
    an._densityElectronRatio = 0.5
    table = an.atomTypeRadialProfiles(2.0, 4, numSD=2.0)
    assert dens.calls == [(8, 2.0, 4, 0.25 + 2.0 * 0.5)]          # ONE device call over the eight eligible atoms
    rows = {row[0]: dict(zip(an.atomTypeRadialProfileHeader, row)) for row in table}
    assert [row[0] for row in table] == sorted(rows) == ["C.syn.alpha", "C.syn.methyl", "N.syn.amide", "O.syn.carbonyl"]
    outer = [0.5, 1.0, 1.5, 2.0]
    for row in rows.values():
        assert row["shell_outer_radius"] == outer
    n = rows["N.syn.amide"]
    assert n["num_atoms"] == 3 and n["optimized_radius"] == 0.78 and n["profile_radius"] == 1.5
    assert np.allclose(n["median_cumulative_density_per_electron"], [0.1, 0.3, 0.6, 0.8], rtol=1e-15, atol=0)
    ca = rows["C.syn.alpha"]
    assert ca["num_atoms"] == 2 and ca["profile_radius"] is None
    assert np.allclose(ca["median_cumulative_density_per_electron"], [0.15, 0.2, 0.3, 0.35], rtol=1e-15, atol=0)
    cb = rows["C.syn.methyl"]
    assert cb["num_atoms"] == 1 and cb["profile_radius"] == 0.5 and cb["median_cumulative_density_per_electron"] == [0.5, 0.5, 0.5, 0.5]
    ox = rows["O.syn.carbonyl"]
    assert ox["num_atoms"] == 2 and ox["profile_radius"] == 2.0 and ox["median_cumulative_density_per_electron"] == [0.0, 0.0, 0.0, 0.5]


def test_atom_profile_rows_on_canned_shells():
    from pdb_eda_amd import singleStructure
    an, dens, spec, sum_sig = _canned_analysis()
    table = an.calculateAtomRadialProfiles(2.0, 4)
    assert dens.calls == [(len(spec), 2.0, 4, 0.25 + 1.5 * 0.5)] and len(table) == len(spec)
    header = an.atomRadialProfileHeader
    for i, (row, (het, num, name, occ)) in enumerate(zip(table, spec)):
        r = dict(zip(header, row))
        assert (r["residue_number"], r["atom_name"], r["occupancy"], r["bfactor"], r["valid"]) == (num, name, occ, 10.0 + i, True)
        assert (r["atom_type"] is None) == (name == "XX9") and (r["electrons"] is None) == (name == "XX9")
        assert r["shell_voxels"] == [3, 3, 3, 3] and r["shell_significant_voxels"] == [2, 2, 2, 2]
        assert r["shell_significant_density"] == sum_sig[i].tolist() and r["shell_density"] == (sum_sig[i] + 1.0).tolist()
        assert all(isinstance(r[k], list) for k in header[-4:])
    only = an.calculateAtomRadialProfiles(2.0, 4, type="CB")
    assert len(only) == 1 and only[0][4] == "CB" and only[0][6] == "C.syn.methyl" and only[0][7] == 9.0
    # the single-structure tables carry the list columns through JSON and CSV
    import json
    an._densityElectronRatio = 0.5
    for level in ("atom", "atom-type"):
        head, rows = singleStructure.rows(an, "profile", level, radius=2.0, shells=4)
        assert json.loads(singleStructure.dumps(head, rows, "json")) == [dict(zip(head, row)) for row in rows]
        text = singleStructure.dumps(head, rows, "csv").splitlines()
        assert text[0] == ",".join(head) and text[1:] == [",".join(map(str, row)) for row in rows]
