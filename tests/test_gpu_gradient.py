"""pdbeda_atom_moments on the MI355X path against tests/gradient_checker.py, the plain numpy restatement of the contract in include/pdbeda.h.
n_voxels with ==; every moment within the bound the checker derives per output (N 2^-(S+1) + c 2^-52 sum|t|: its docstring); the exact
properties -- zeros as +0.0, runs, permutations, an atom alone, coincident atoms, the unique-box flag -- to the byte; the counters against
the plan's restatement; ADJOINTNESS against pdbeda_model_density, which ties the pair sets of the two kernels to each other; and every
refusal, after which the context stays usable.  On orthogonal cells the checker takes the voxel coordinates from the header's own
crs2xyzCoord; only on the skewed cell, where the host's np.dot is not pinned to the bit, from the device's crs2xyz, which
tests/test_gpu_voxel.py pins."""
import io
import math

import numpy as np
import pytest

import gradient_cases as cases
import gradient_checker as checker

pytestmark = pytest.mark.gpu

_maps, _wanted = {}, {}
CASES = cases.cases()
IDS = [c[0] for c in CASES]


def device_map(name, gpu_ctx, kind="zero", grid=None, tag=None):
    """A DensityMatrix on the geometry ``name`` holding the weight map ``kind`` (or ``grid`` under ``tag``)."""
    from pdb_eda_amd import ccp4, synthetic
    key = (name, kind if tag is None else tag)
    if key not in _maps:
        data = cases.weight(name, kind) if grid is None else grid
        _maps[key] = (ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(cases.spec_of(name), data)), name, ctx=gpu_ctx), data)
    return _maps[key]


def where_of(dm):
    return None if dm.header.orthogonal else dm._map.crs2xyz


def wanted(case, dm, data):
    """The checker's answer, computed once per case and shared (never modified)."""
    tag, name, kind, unique, xyz, expo, radii = case
    if tag not in _wanted:
        _wanted[tag] = checker.moments(dm.header, data, xyz, expo, radii, unique=unique, key=name, crs2xyz=where_of(dm))
    return _wanted[tag]


def plus_zero(a):
    return np.all(np.ascontiguousarray(a).view(np.uint64) == 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_checker(gpu_ctx, case):
    tag, name, kind, unique, xyz, expo, radii = case
    dm, data = device_map(name, gpu_ctx, kind)
    want = wanted(case, dm, data)
    got = dm.atomMoments(xyz, expo, radii, uniqueBox=unique)
    shift, v_max, clipped, boxes = checker.plan(dm.header, xyz, radii, float(np.abs(data).max()), unique)
    assert got["counters"] == {"shift": shift, "maxBoxVoxels": v_max, "clippedAtoms": clipped}, tag
    assert got["nVoxels"].dtype == np.int32 and np.array_equal(got["nVoxels"], want["nVoxels"]), tag
    assert got["moments"].shape == (len(xyz), expo.shape[1], 5)
    err, bound = np.abs(got["moments"] - want["exact"]), checker.bounds(want, shift)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: S %d, V_max %d, clipped %d, pairs %d, max |out - exact| / bound = %.3g, E_max %.3g"
          % (tag, shift, v_max, clipped, int(want["nVoxels"].sum()), float(ratio.max()), want["e_max"]))
    assert np.all(err <= bound), tag
    empty = want["nVoxels"] == 0
    assert (empty.any() or tag.startswith("wide-trips")) and (want["nVoxels"] > 0).any(), tag      # (atoms wholly outside; and not vacuous)
    assert plus_zero(got["moments"][empty]), tag                                               # exactly +0.0
    if kind == "zero":
        assert plus_zero(got["moments"]), tag
    # two calls, a permuted list (rows re-mapped) and coincident atoms: the same bytes
    again = dm.atomMoments(xyz, expo, radii, uniqueBox=unique)
    assert again["moments"].tobytes() == got["moments"].tobytes() and again["nVoxels"].tobytes() == got["nVoxels"].tobytes(), tag
    perm = np.random.default_rng(29).permutation(len(xyz))
    moved = dm.atomMoments(xyz[perm], expo[perm], radii[perm], uniqueBox=unique)
    assert moved["moments"].tobytes() == got["moments"][perm].tobytes() and np.array_equal(moved["nVoxels"], got["nVoxels"][perm]), tag
    assert moved["counters"] == got["counters"], tag


def test_coincident_atoms_have_identical_rows(gpu_ctx):
    tag, name, kind, unique, xyz, expo, radii = cases.find("box-1term-random")
    dm, _ = device_map(name, gpu_ctx, kind)
    assert np.array_equal(xyz[14], xyz[15]) and radii[14] == radii[15]
    expo = expo.copy()
    expo[15] = expo[14]
    got = dm.atomMoments(xyz, expo, radii)
    assert got["moments"][14].tobytes() == got["moments"][15].tobytes() and got["nVoxels"][14] == got["nVoxels"][15] > 0


def test_an_atom_alone_agrees_with_itself_among_the_others(gpu_ctx):
    """S ties the atoms of a call through r_max and V_max only: the atom of the largest radius and box, alone, is computed at the same S."""
    tag, name, kind, unique, xyz, expo, radii = cases.find("skew-3term-random")
    dm, _ = device_map(name, gpu_ctx, kind)
    full = dm.atomMoments(xyz, expo, radii)
    k = int(np.argmax(radii))
    alone = dm.atomMoments(xyz[k:k + 1], expo[k:k + 1], radii[k:k + 1])
    assert alone["counters"]["shift"] == full["counters"]["shift"] and alone["nVoxels"][0] == full["nVoxels"][k] > 0
    assert alone["moments"][0].tobytes() == full["moments"][k].tobytes()
    for k in (0, 7, 16):                                                                     # smaller atoms: V_max stays below 2^22, r_max^2 in the same binade or below 1
        alone = dm.atomMoments(xyz[k:k + 1], expo[k:k + 1], radii[k:k + 1])
        if alone["counters"]["shift"] == full["counters"]["shift"]:
            assert alone["moments"][0].tobytes() == full["moments"][k].tobytes()
        else:                                                                                # a finer quantum: within the coarser one's roundings
            assert np.all(np.abs(alone["moments"][0] - full["moments"][k]) <= (full["nVoxels"][k] + 1) * 2.0 ** -full["counters"]["shift"])


def test_the_unique_box_flag_equals_a_map_zeroed_outside_it(gpu_ctx):
    """On ``rep`` (21 stored columns, 16 unique) the flag changes the answer; it equals the unflagged call on a map zeroed outside the unique box.
    The largest |w| is put inside the unique box, so both calls have one S: asserted."""
    name = "rep"
    xyz, expo, radii = cases.atoms(name, 3)
    w = cases.weight(name, "random").copy()
    w[0, 0, 0] = np.float32(1.0)
    cut = w.copy()
    cut[:, :, 16:] = 0.0
    a, _ = device_map(name, gpu_ctx, grid=w, tag="flag-full")
    b, _ = device_map(name, gpu_ctx, grid=cut, tag="flag-cut")
    assert list(a.header.uniqueNcrs) == [16, 9, 7] and list(a.header.ncrs) == [21, 9, 7]
    flagged, plain, zeroed = a.atomMoments(xyz, expo, radii, uniqueBox=True), a.atomMoments(xyz, expo, radii), b.atomMoments(xyz, expo, radii)
    assert flagged["counters"]["shift"] == zeroed["counters"]["shift"] == plain["counters"]["shift"]
    assert flagged["moments"].tobytes() == zeroed["moments"].tobytes()
    assert flagged["moments"].tobytes() != plain["moments"].tobytes() and np.any(flagged["nVoxels"] < plain["nVoxels"])
    assert np.all(flagged["nVoxels"] <= plain["nVoxels"]) and np.array_equal(plain["nVoxels"], zeroed["nVoxels"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_adjointness_with_the_model_density(gpu_ctx, case):
    """sum_a sum_j amp M0 from atomMoments(w) against sum_v w(v) model(v) from the downloaded modelDensity of the same atoms: <w, A amp> = <A^T w,
    amp>.  The tolerance is the two calls' own bounds: the checker's bound of every M0 times |amp|, plus ONE float32 spacing of the model's voxel
    times |w(v)| (the model's contract: half a spacing for its last rounding, and its integer roundings below a thousandth of that), plus the
    fp64 rounding of the two host-side products (2^-52 of the sums of magnitudes)."""
    tag, name, kind, unique, xyz, expo, radii = case
    dm, data = device_map(name, gpu_ctx, kind)
    want = wanted(case, dm, data)
    amp = cases.model_terms(xyz, expo, radii)
    got = dm.atomMoments(xyz, expo, radii, uniqueBox=unique)
    model = dm.modelDensity(xyz, amp, expo, radii).density.astype(np.float64)
    w = data.astype(np.float64)
    if unique:
        uc, ur, us = (int(v) for v in dm.header.uniqueNcrs)
        model, w = model[:us, :ur, :uc], w[:us, :ur, :uc]
    m0 = got["moments"][:, :, 0]
    left = math.fsum((amp * m0).reshape(-1).tolist())
    right = math.fsum((w * model).reshape(-1).tolist())
    spacing = np.abs(np.spacing(model.astype(np.float32))).astype(np.float64)
    tol = (math.fsum((np.abs(amp) * checker.bounds(want, got["counters"]["shift"])[:, :, 0]).reshape(-1).tolist())
           + math.fsum((np.abs(w) * spacing).reshape(-1).tolist())
           + 2.0 ** -52 * (math.fsum(np.abs(amp * m0).reshape(-1).tolist()) + math.fsum(np.abs(w * model).reshape(-1).tolist())))
    print("%s: sum amp M0 = %.17g, sum w model = %.17g, |difference| = %.3g, tolerance %.3g" % (tag, left, right, abs(left - right), tol))
    assert abs(left - right) <= tol, tag
    if kind != "zero":
        assert right != 0.0 and tol < 1e-3 * math.fsum(np.abs(w * model).reshape(-1).tolist()), tag      # (the tolerance decides something)


def test_refusals_leave_the_context_usable(gpu_ctx):
    """Every refusal of the contract raises PDBEDA_ERR_ARGUMENT and the next call computes the same bytes.  One refusal cannot be reached here: a
    clipped box of 2^31 voxels needs a map that large; tests/test_gradient_plan_host.py covers it in the plan."""
    from pdb_eda_amd import _native
    tag, name, kind, unique, xyz, expo, radii = cases.find("box-3term-random")
    dm, data = device_map(name, gpu_ctx, kind)
    good = dm.atomMoments(xyz, expo, radii)

    def refused(call):
        with pytest.raises(_native.PdbedaError) as info:
            call()
        assert info.value.code == _native.PDBEDA_ERR_ARGUMENT
        again = dm.atomMoments(xyz, expo, radii)                                             # the context works, and computes the same
        assert again["moments"].tobytes() == good["moments"].tobytes()

    def with_value(array, at, value):
        out = np.array(array, copy=True)
        out.reshape(-1)[at] = value
        return out

    refused(lambda: dm.atomMoments(xyz, np.zeros((len(xyz), 7)), radii))                      # n_terms out of range
    for bad in (np.nan, np.inf, -np.inf):
        refused(lambda: dm.atomMoments(with_value(xyz, 4, bad), expo, radii))                # a non-finite coordinate
        refused(lambda: dm.atomMoments(xyz, with_value(expo, 5, bad), radii))                # a non-finite exponent
        refused(lambda: dm.atomMoments(xyz, expo, with_value(radii, 2, bad)))                # a radius that is not finite
    refused(lambda: dm.atomMoments(xyz, with_value(expo, 5, -1e-300), radii))                # a negative exponent
    refused(lambda: dm.atomMoments(xyz, expo, with_value(radii, 2, 0.0)))                    # a radius <= 0
    refused(lambda: dm.atomMoments(xyz, expo, with_value(radii, 2, -1.0)))
    refused(lambda: dm.atomMoments(xyz, expo, with_value(radii, 2, 3.0e8)))                  # 2^29 grid steps of 0.5 A or more
    lib, h = dm._ctx._lib, dm._map._h
    args = (_native._ptr(np.ascontiguousarray(xyz)), len(xyz), 3, _native._ptr(np.ascontiguousarray(expo)), _native._ptr(np.ascontiguousarray(radii)))
    refused(lambda: dm._ctx.check(lib.pdbeda_atom_moments(h, *args, 2, None, None, None), "pdbeda_atom_moments"))          # an unknown flag
    refused(lambda: dm._ctx.check(lib.pdbeda_atom_moments(h, args[0], 2 ** 31, 3, args[3], args[4], 0, None, None, None), "pdbeda_atom_moments"))   # 2^31 atoms (refused before an array is read)
    # a weight map with a non-finite voxel, as the labelling calls refuse it
    holed = data.copy()
    holed[1, 2, 3] = np.nan
    bad_map, _ = device_map(name, gpu_ctx, grid=holed, tag="holed")
    with pytest.raises(_native.PdbedaError) as info:
        bad_map.atomMoments(xyz, expo, radii)
    assert info.value.code == _native.PDBEDA_ERR_ARGUMENT
    # a failing call leaves the outputs untouched
    moments, n_vox, ctr = np.full((len(xyz), 3, 5), 7.0), np.full(len(xyz), 7, dtype=np.int32), np.full(3, 7, dtype=np.int64)
    rc = lib.pdbeda_atom_moments(h, *args, 2, _native._ptr(moments), _native._ptr(n_vox), _native._ptr(ctr))
    assert rc == _native.PDBEDA_ERR_ARGUMENT and np.all(moments == 7.0) and np.all(n_vox == 7) and np.all(ctr == 7)
    # the empty call succeeds and touches nothing
    rc = lib.pdbeda_atom_moments(h, None, 0, 1, None, None, 0, _native._ptr(moments), _native._ptr(n_vox), _native._ptr(ctr))
    assert rc == 0 and np.all(moments == 7.0) and np.all(n_vox == 7) and np.all(ctr == 7)
    empty = dm.atomMoments(np.zeros((0, 3)), np.zeros((0, 1)), np.zeros(0, dtype=np.float32))
    assert empty["moments"].shape == (0, 1, 5) and len(empty["nVoxels"]) == 0
    assert dm.atomMoments(xyz, expo, radii)["moments"].tobytes() == good["moments"].tobytes()
