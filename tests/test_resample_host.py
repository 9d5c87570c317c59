"""tests/resample_checker.py -- the numpy restatement of pdbeda_map_resample that tests/test_gpu_resample.py holds the device to, bit for
bit -- against scipy and against identities that hold exactly; the host helpers of ``ccp4`` (operators, Kabsch, destination headers);
and the guard that keeps the bit comparisons from being vacuous.  No GPU."""
import numpy as np
import pytest

from pdb_eda_amd import ccp4

import resample_cases as rc
import resample_checker as chk

EPS = float(np.finfo(np.float64).eps)


def periodic_positions(seed=3, n=400):
    """Coordinates all over (and beyond) the periodic ``box`` map, their grid positions, and the map."""
    header, grid = rc.header_of("box"), rc.grid_of("box")
    lo, hi = rc.model_cases.box_of("box")
    xyz = np.random.default_rng(seed).uniform(lo - 3.0, hi + 3.0, size=(n, 3))
    return header, grid, chk.snap(chk.xyz2frac(header, xyz))


def test_order_one_is_scipy_grid_wrap():
    from scipy.ndimage import map_coordinates
    header, grid, f = periodic_positions()
    got, valid = chk.sample(header, grid, f, 1)
    want = map_coordinates(grid.astype(np.float64), [f[:, 2], f[:, 1], f[:, 0]], order=1, mode="grid-wrap")
    assert valid.all()
    assert float(np.abs(got - want).max()) <= 32 * EPS * float(np.abs(grid).max())


def test_order_zero_is_scipy_nearest():
    from scipy.ndimage import map_coordinates
    header, grid, f = periodic_positions(seed=4)
    got, valid = chk.sample(header, grid, f, 0)
    want = map_coordinates(grid.astype(np.float64), [f[:, 2], f[:, 1], f[:, 0]], order=0, mode="grid-wrap")
    assert valid.all() and np.array_equal(got, want)


def test_cubic_weights_sum_to_one():
    t = np.concatenate([np.linspace(0.0, 1.0, 1001)[:-1], np.random.default_rng(0).uniform(0.0, 1.0, 1000)])
    w = chk.cubic_weights(t)
    assert float(np.abs(((w[0] + w[1]) + w[2]) + w[3] - 1.0).max()) <= 4 * EPS
    at0 = chk.cubic_weights(np.zeros(1))
    assert [float(v[0]) for v in at0] == [0.0, 1.0, 0.0, 0.0]


def test_order_three_reproduces_a_linear_field():
    """Catmull-Rom interpolates a linear function exactly: on a cut-out large enough to hold every support, a field a + b . crs comes
    back within the bound of the order-1 comparison."""
    header = rc.spec_header(ncrs=(24, 20, 16), interval=(48, 40, 32), spacing=0.5)
    s, r, c = np.meshgrid(np.arange(16), np.arange(20), np.arange(24), indexing="ij")
    grid = (0.25 + 0.5 * c - 0.125 * r + 0.375 * s).astype(np.float32)      # (exact in float32)
    f = np.random.default_rng(9).uniform([1.0, 1.0, 1.0], [21.0, 17.0, 13.0], size=(500, 3))
    got, valid = chk.sample(header, grid, f, 3)
    want = 0.25 + 0.5 * f[:, 0] - 0.125 * f[:, 1] + 0.375 * f[:, 2]
    assert valid.all()
    assert float(np.abs(got - want).max()) <= 32 * EPS * float(np.abs(grid).max())


@pytest.mark.parametrize("order", rc.ORDERS)
@pytest.mark.parametrize("name", rc.SOURCES)
def test_identity_returns_the_map(name, order):
    """The identity onto the map's own header: every voxel, the faces of a cut-out included (the snap puts a position that is 1e-13 beside
    a voxel ON it, and t == 0 then asks for that voxel alone)."""
    header, grid = rc.header_of(name), rc.grid_of(name)
    out, count = chk.resample(header, grid, header, rc.IDENTITY, order, fill=np.nan)
    assert (count == 1).all() and out.tobytes() == grid.tobytes()


@pytest.mark.parametrize("order", rc.ORDERS)
def test_whole_grid_steps_roll_the_map(order):
    header, grid = rc.header_of("box"), rc.grid_of("box")
    out, count = chk.resample(header, grid, header, rc.grid_shift(header, (5, -2, 3)), order)
    assert (count == 1).all() and out.tobytes() == np.roll(grid, (-3, 2, -5), axis=(0, 1, 2)).tobytes()


@pytest.mark.parametrize("order", rc.ORDERS)
def test_two_fold_flips_the_map(order):
    """x -> -x, y -> -y on an orthogonal full cell whose origin is a grid point: voxel (c, r, s) reads (-c, -r, s), the flipped array
    rolled by one."""
    header, grid = rc.header_of("box"), rc.grid_of("box")
    two_fold = np.hstack([np.diag([-1.0, -1.0, 1.0]), np.zeros((3, 1))])
    out, count = chk.resample(header, grid, header, two_fold, order)
    want = np.roll(grid[:, ::-1, ::-1], (1, 1), axis=(1, 2))
    assert (count == 1).all() and out.tobytes() == want.tobytes()


def test_validity_needs_only_the_used_voxels():
    """On the last stored column of a cut-out (t == 0 along c) the sample is valid though column n is not stored; half a step further it is not."""
    header, grid = rc.header_of("skew"), rc.grid_of("skew")
    nc = int(header.ncrs[0])
    f = np.array([[nc - 1.0, 2.0, 3.0], [nc - 0.5, 2.0, 3.0], [nc - 1.0, 0.5, 3.0]])      # (the third: rows 0 and 1 at order 1, rows -1 .. 2 at order 3)
    for order in (1, 3):
        value, valid = chk.sample(header, grid, f, order)
        assert valid.tolist() == [True, False, order == 1]
        assert value[0] == float(grid[3, 2, nc - 1])


def test_kabsch_recovers_a_rigid_motion_and_refuses_a_reflection():
    rng = np.random.default_rng(12)
    p = rng.normal(size=(25, 3)) * 6.0
    want = rc.rigid((0.4, -0.7, 1.1), (1.0, 2.0, 3.0), (4.0, -5.0, 6.0))
    q = ccp4.applyOperator(want, p)
    op, rmsd = ccp4.kabschOperator(p, q)
    assert float(np.abs(op - want).max()) < 1e-12 and rmsd < 1e-12
    weights = rng.uniform(0.5, 2.0, 25)
    noisy = q + rng.normal(size=q.shape) * 0.05
    op_w, rmsd_w = ccp4.kabschOperator(p, noisy, weights)
    assert float(np.abs(op_w - want).max()) < 0.05 and 0.0 < rmsd_w < 0.2
    mirrored = q * np.array([-1.0, 1.0, 1.0])
    op_m, rmsd_m = ccp4.kabschOperator(p, mirrored)
    assert abs(float(np.linalg.det(op_m[:, :3])) - 1.0) < 1e-12 and rmsd_m > 1.0          # a rotation all the same, and a poor fit
    assert float(np.abs(op_m[:, :3].dot(op_m[:, :3].T) - np.eye(3)).max()) < 1e-12
    with pytest.raises(ValueError):
        ccp4.kabschOperator(p[:2], q[:2])


def test_operators_round_trip():
    a, b = rc.rigid((0.3, 0.2, -0.9), (1.0, 0.0, 2.0), (0.5, 1.5, -2.5)), rc.rigid((-1.2, 0.4, 0.1), (0.0, 3.0, 1.0), (2.0, 0.0, 1.0))
    x = np.random.default_rng(1).normal(size=(7, 3))
    assert np.array_equal(ccp4.identityOperator(), np.hstack([np.eye(3), np.zeros((3, 1))]))
    assert float(np.abs(ccp4.applyOperator(ccp4.composeOperators(a, b), x) - ccp4.applyOperator(a, ccp4.applyOperator(b, x))).max()) < 1e-13
    assert float(np.abs(ccp4.composeOperators(a, ccp4.invertOperator(a)) - ccp4.identityOperator()).max()) < 1e-14
    assert float(np.abs(ccp4.composeOperators(ccp4.invertOperator(a), a) - ccp4.identityOperator()).max()) < 1e-14
    assert float(np.abs(ccp4.invertOperator(ccp4.invertOperator(b)) - b).max()) < 1e-14


@pytest.mark.parametrize("centre, half, spacing", [((10.3, -4.2, 7.7), (3.0, 4.0, 5.0), 0.25), ((-31.07, 0.0, 55.5), 2.2, 0.3), ((0.0, 0.0, 0.0), (1.0, 0.0, 2.5), (0.2, 0.7, 0.11))])
def test_box_header_covers_what_was_asked(centre, half, spacing):
    header = ccp4.boxHeader(centre, half, spacing)
    assert isinstance(header, ccp4.DensityHeader) and header.orthogonal and header.geometry().ncrs[0] == header.ncrs[0]
    lo, hi = np.array(header.crs2xyzCoord([0, 0, 0])), np.array(header.crs2xyzCoord([n - 1 for n in header.ncrs]))
    centre, half = np.asarray(centre, dtype=np.float64), np.broadcast_to(np.asarray(half, dtype=np.float64), (3,))
    step = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    assert (lo <= centre - half).all() and (hi >= centre + half).all()
    assert (lo > centre - half - 1.001 * step).all() and (hi < centre + half + 1.001 * step).all()          # and no more than a step beyond
    assert all(header.xyzInterval[k] >= header.ncrs[k] for k in range(3))                                   # the cell holds the box
    assert all(float(np.float32(v)) == v for v in header.xyzLength)                                         # the lengths survive a CCP4 header
    assert float(np.abs(np.array(header.gridLength) / step - 1.0).max()) < 2.0 ** -23
    origin_steps = np.array(header.origin) / np.array(header.gridLength)
    assert float(np.abs(origin_steps - np.rint(origin_steps)).max()) < 1e-9                                 # crsStart lies on the grid


@pytest.mark.parametrize("name", rc.SOURCES)
def test_cell_header_is_the_whole_cell(name):
    header = rc.header_of(name)
    cell = ccp4.cellHeader(header)
    assert isinstance(cell, ccp4.DensityHeader) and list(cell.ncrs) == list(header.crsInterval) and list(cell.crsStart) == [0, 0, 0]
    assert list(cell.xyzInterval) == list(header.xyzInterval) and list(cell.xyzLength) == list(header.xyzLength) and cell.map2crs == header.map2crs
    assert np.array_equal(np.asarray(cell.orthoMat, dtype=np.float64), np.asarray(header.orthoMat, dtype=np.float64)) and cell.orthogonal == header.orthogonal
    g = cell.geometry()
    assert [g.ncrs[k] for k in range(3)] == list(header.crsInterval)
    # a voxel of the cut-out and the voxel of the cell it is a copy of lie a whole number of cells apart
    at = [2, 1, 3]
    in_cell = [(at[k] + header.crsStart[k]) % header.crsInterval[k] for k in range(3)]
    delta = np.asarray(header.deOrthoMat, dtype=np.float64).dot(np.array(header.crs2xyzCoord(at)) - np.array(cell.crs2xyzCoord(in_cell)))
    assert float(np.abs(delta - np.rint(delta)).max()) < 1e-9


@pytest.mark.parametrize("order", rc.ORDERS)
@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_no_case_is_vacuous(name, order):
    """By the checker alone: a quarter of every destination is covered and holds magnitudes above 0.1, and a tenth of every cut-out case is not covered."""
    strong, uncovered = rc.guard(name, order)
    assert strong >= 0.25, (name, order, strong)
    if rc.cases()[name]["cutout"]:
        assert uncovered >= 0.1, (name, order, uncovered)


def test_budget_cases_straddle_the_budget():
    """The largest staged box of the one case is just inside the LDS budget; the full tiles of the other are just outside it, its clipped tiles inside."""
    inside = rc.tile_footprints(rc.cases()["budget-inside"], 3)
    outside = rc.tile_footprints(rc.cases()["budget-outside"], 3)
    assert 0.8 * rc.LDS_VOX < inside.max() <= rc.LDS_VOX
    assert rc.LDS_VOX < outside.max() <= 1.25 * rc.LDS_VOX and outside.min() <= rc.LDS_VOX
