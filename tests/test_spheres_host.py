"""The per-atom region-sum yardstick without a GPU: the numpy checker (tests/spheres_checker.py, what
tests/test_gpu_batch_limits.py compares the device with) tied to the pinned oracle -- its sphere lists, its validity test and
its point densities -- on the voxel goldens, with the atoms of the radial-profile tests (inside, at the edges of and outside
the stored box, and exactly on voxel centres)."""
import numpy as np
import pytest

from conftest import crs_set, load_case
import profiles_cases
import spheres_checker

CASES = ["orth", "orth_sub", "hex", "tric"]
RADII = [0.7, 1.9, 3.5]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    from oracle import oracle as ora
    z, header, grid = load_case(request.param)
    return request.param, z, header, grid, ora.Oracle(header, grid), profiles_cases.case_atoms(request.param, header)


def _oracle_density(o, voxels):
    return np.array([o.point_density(v) for v in np.asarray(voxels).reshape(-1, 3)], dtype=np.float64)


def _oracle_sums(d, cutoff):
    """fp64 sums of Oracle.point_density over a voxel list: (pos, neg) with the strict comparisons against float32(cutoff)."""
    cut = float(np.float32(cutoff))
    return float(np.sum(d[d > cut])), float(np.sum(d[d < -cut]))


def _assert_sums(got, g, want_pos, want_neg, what):
    for mine, theirs in ((got["pos"][g], want_pos), (got["neg"][g], want_neg)):
        assert abs(mine - theirs) <= 1e-12 * abs(theirs), what          # (terms of one sign: no cancellation; an empty sum is exactly 0)


@pytest.mark.parametrize("radius", RADII)
def test_per_atom_against_the_oracle(case, radius):
    name, z, header, grid, o, xyz = case
    assert len(xyz) == 32
    sigma = float(z["mean"]) + 1.5 * float(z["std"])
    spheres = spheres_checker.atom_spheres(header, grid, xyz, radius)
    members = spheres_checker.group_voxels(spheres)
    plain = spheres_checker.region_sums(header, grid, xyz, radius, 0.0, spheres=spheres)
    cut = spheres_checker.region_sums(header, grid, xyz, radius, sigma, spheres=spheres)
    assert plain["cnt"].sum() > 0 and np.array_equal(plain["cnt"], cut["cnt"]) and np.array_equal(plain["valid"], cut["valid"])
    assert np.all(np.abs(cut["pos"]) <= np.abs(plain["pos"])) and np.any(cut["pos"] != plain["pos"])
    for a, p in enumerate(xyz):
        want = o.sphere_crs(p, radius, 0.0)
        assert plain["cnt"][a] == len(want) and members[a] == crs_set(want), (name, radius, a)
        assert bool(plain["valid"][a]) == o.valid_xyz(p, radius), (name, radius, a)
        d = _oracle_density(o, want)
        for got, c in ((plain, 0.0), (cut, sigma)):
            _assert_sums(got, a, *_oracle_sums(d, c), what=(name, radius, a, c))
    if name in ("orth_sub", "hex"):          # stored voxels missing from the cell: both answers occur
        assert plain["valid"].any() and not plain["valid"].all()


def test_grouped_against_the_oracle(case):
    """Groups of 1, 4 and 9 atoms (drawn from the case's atoms, so that the spheres of a group overlap, touch or lie apart),
    a radius per atom: the union is a set on raw crs, `valid` the conjunction over the group's atoms."""
    name, z, header, grid, o, xyz = case
    sizes = [1, 4, 9, 9, 4, 1, 4]
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert goff[-1] == len(xyz)
    # the first three groups take the case's atoms as they are (mostly far apart); in the other four every atom but the group's first
    # sits 1.2 A from the one before it, so spheres of 0.7 .. 3.5 A share voxels
    xyz = xyz.copy()
    for g in range(3, len(sizes)):
        for a in range(int(goff[g]) + 1, int(goff[g + 1])):
            xyz[a] = xyz[a - 1] + np.array([0.7, -0.6, 0.77])
    radii = np.array([RADII[a % 3] for a in range(len(xyz))], dtype=np.float32)
    sigma = float(z["mean"]) + 1.5 * float(z["std"])
    spheres = spheres_checker.atom_spheres(header, grid, xyz, radii)
    members = spheres_checker.group_voxels(spheres, goff)
    shared = 0
    for c in (0.0, sigma):
        got = spheres_checker.region_sums(header, grid, xyz, radii, c, group_offsets=goff, spheres=spheres)
        for g in range(len(sizes)):
            a, b = int(goff[g]), int(goff[g + 1])
            want = o.sphere_crs_list(xyz[a:b], radii[a:b], 0.0) if b - a > 1 else o.sphere_crs(xyz[a], radii[a], 0.0)
            assert got["cnt"][g] == len(want) and members[g] == crs_set(want), (name, g)
            assert bool(got["valid"][g]) == all(o.valid_xyz(xyz[i], radii[i]) for i in range(a, b)), (name, g)
            _assert_sums(got, g, *_oracle_sums(_oracle_density(o, want), c), what=(name, g, c))
            shared += int(np.diff(spheres["offsets"])[a:b].sum()) - len(want)
    assert shared > 0          # voxels that two atoms of a group reached were counted once
    assert got["cnt"].sum() > 0
