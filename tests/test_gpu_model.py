"""The model density and the pair moments on the MI355X path against tests/model_checker.py, the plain numpy restatement of the contracts
in include/pdbeda.h (pdbeda_model_density, pdbeda_map_pair_moments).  Every voxel of a calculated map lies within one float32 spacing of
the exact value (tests/model_cases.py says why the cases allow that), an unreached voxel is exactly +0.0, and runs and permutations agree to
the bit; the five sums agree within 1e-9 of the sum of their absolute terms.  On orthogonal cells the checker takes the voxel
coordinates from the header's own crs2xyzCoord, so nothing in the reference is native; only on the skewed cell, where the host's np.dot
is not pinned to the bit, from the device's crs2xyz, which tests/test_gpu_voxel.py pins."""
import ctypes
import io
import math

import numpy as np
import pytest

from conftest import load_analysis_case
import model_cases
import model_checker

pytestmark = pytest.mark.gpu

STAGE = model_cases.STAGE
_maps, _wanted = {}, {}


def device_map(name, gpu_ctx, grid=None, tag=""):
    """A DensityMatrix on the geometry ``name`` (zeros unless a grid is given)."""
    from pdb_eda_amd import ccp4, synthetic
    key = (name, tag)
    if key not in _maps:
        spec = model_cases.spec_of(name)
        nc, nr, ns = spec.ncrs
        data = np.zeros((ns, nr, nc), dtype=np.float32) if grid is None else grid
        _maps[key] = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, data)), name, ctx=gpu_ctx)
    return _maps[key]


def where_of(dm):
    """Where the checker takes its voxel coordinates from: on orthogonal cells the header's own crs2xyzCoord (nothing native in the
    reference at all); on skewed cells, whose host np.dot is not pinned to the bit, the device's crs2xyz, which tests/test_gpu_voxel.py pins."""
    return None if dm.header.orthogonal else dm._map.crs2xyz


def checker(tag, dm, atoms):
    """The checker's answer, computed once per case and shared (never modified)."""
    if tag not in _wanted:
        _wanted[tag] = model_checker.density(dm.header, *atoms, crs2xyz=where_of(dm))
    return _wanted[tag]


def assert_density(got, want, what):
    """got: the downloaded float32 map;  want: model_checker.density()."""
    exact = want["exact"]
    assert got.dtype == np.float32 and got.shape == exact.shape, what
    err, bound = np.abs(got.astype(np.float64) - exact), np.abs(np.spacing(exact.astype(np.float32))).astype(np.float64)      # (the spacing of a negative float is negative)
    worst = int(np.argmax(err / bound))
    print("%s: max |out - exact| / float32 spacing = %.3g (at a voxel of %d atoms, exact %.9g); %d of %d voxels reached"
          % (what, float((err / bound).reshape(-1)[worst]), int(want["count"].reshape(-1)[worst]), float(exact.reshape(-1)[worst]),
             int((want["count"] > 0).sum()), exact.size))
    assert np.all(err <= bound), what
    untouched = want["count"] == 0
    assert np.all(got[untouched].view(np.uint32) == 0), what          # exactly +0.0f


def run_case(dm, tag, atoms, want_multi=None):
    xyz, amp, expo, radii = atoms
    want = checker(tag, dm, atoms)
    out = dm.modelDensity(xyz, amp, expo, radii)
    got = out.density
    assert_density(got, want, tag)
    ctr = out.modelCounters
    assert ctr["shift"] == model_checker.shift_rule(len(xyz), model_checker.a_max(model_checker.terms_2d(amp, len(xyz)))) == 40      # (fewer gridded atoms change nothing below 2^22)
    print("%s: counters %s" % (tag, ctr))
    if want_multi is not None:
        assert (ctr["multiRunTiles"] > 0) == want_multi, (tag, ctr)
    again = dm.modelDensity(xyz, amp, expo, radii)
    assert again.density.tobytes() == got.tobytes(), tag
    perm = np.random.default_rng(23).permutation(len(xyz))
    amp2, expo2 = model_checker.terms_2d(amp, len(xyz)), model_checker.terms_2d(expo, len(xyz))
    moved = dm.modelDensity(xyz[perm], amp2[perm], expo2[perm], radii[perm])
    assert moved.density.tobytes() == got.tobytes(), tag
    return out, ctr


@pytest.mark.parametrize("name", ["box", "skew", "rep", "tile", "past"])
@pytest.mark.parametrize("n_terms", [1, 6])
def test_scattered_atoms_against_checker(gpu_ctx, name, n_terms):
    """Boxes that are no multiple of the tile, one exact tile, one voxel past it, a skewed cell with permuted axes and a start, a stored box
    larger than the unique one; atoms outside that reach in, far atoms, coincident atoms, radii 4x apart, one and six terms (one negative)."""
    dm = device_map(name, gpu_ctx)
    atoms = model_cases.scattered(name, n_terms=n_terms)
    want = checker("scattered-%s-%d" % (name, n_terms), dm, atoms)
    assert (want["count"] > 0).any() and (want["count"] == 0).any() and want["count"].max() >= 2          # (a vacuous comparison cannot pass)
    out, ctr = run_case(dm, "scattered-%s-%d" % (name, n_terms), atoms, want_multi=False)
    assert 0 < ctr["maxStaged"] <= len(atoms[0]) - 2          # (the two far atoms are never gridded)
    assert list(out.header.ncrs) == list(dm.header.ncrs) and out.density.min() >= 0.0


@pytest.mark.parametrize("n", [STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 3])
def test_both_sides_of_the_staging_buffer(gpu_ctx, n):
    """All atoms inside the first tile: it stages every one of them, in one run up to STAGE and in more beyond."""
    dm = device_map("box", gpu_ctx)
    out, ctr = run_case(dm, "clustered-%d" % n, model_cases.clustered("box", n), want_multi=n > STAGE)
    assert ctr["maxStaged"] == n


def test_neighbouring_tiles_stage_different_atoms(gpu_ctx):
    dm = device_map("wide", gpu_ctx)
    atoms = model_cases.spread()
    out, ctr = run_case(dm, "spread", atoms)
    assert 0 < ctr["maxStaged"] < len(atoms[0]) // 2          # (no tile sees even half of them)


def test_mixed_signs_cancel(gpu_ctx):
    dm = device_map("box", gpu_ctx)
    atoms = model_cases.cancelling("box")
    want = checker("cancelling", dm, atoms)
    dead = (want["count"] > 0) & (want["exact"] == 0.0)
    assert dead.sum() >= 20 and (want["exact"] > 0).sum() >= 20 and want["exact"].min() == 0.0
    out, _ = run_case(dm, "cancelling", atoms)
    assert np.all(out.density[dead].view(np.uint32) == 0)          # +a and -a on one spot: the integers add up to exactly nothing


def test_on_the_sphere_and_a_constant_inside(gpu_ctx):
    """Crafted: orthogonal cell, atom on a voxel centre, radius an exact float32 multiple of the grid step, expo = 0."""
    dm = device_map("box", gpu_ctx)
    atoms = model_cases.on_sphere("box")
    want = model_checker.density(dm.header, *atoms, crs2xyz=where_of(dm))
    assert want["on_sphere"].sum() == 30
    got = dm.modelDensity(*atoms).density
    assert np.all(got[want["on_sphere"]] == np.float32(0.75))
    assert np.array_equal(got, np.where(want["count"] > 0, np.float32(0.75), np.float32(0.0)).astype(np.float32))


def test_no_atoms_is_an_all_zero_map(gpu_ctx):
    dm = device_map("past", gpu_ctx)
    out = dm.modelDensity(np.zeros((0, 3)), np.zeros((0, 1)), np.zeros((0, 1)), np.zeros(0, dtype=np.float32))
    assert out.density.shape == (5, 5, 17) and not out.density.view(np.uint32).any()
    assert out.modelCounters == {"shift": 40, "maxStaged": 0, "multiRunTiles": 0}
    far = dm.modelDensity(np.array([[500.0, 0.0, 0.0]]), [[1.0]], [[1.0]], np.array([2.0], dtype=np.float32))
    assert not far.density.view(np.uint32).any() and far.modelCounters["maxStaged"] == 0


def test_shift_follows_the_amplitudes(gpu_ctx):
    """Amplitudes of 2^30: n A_max = 40 * 2^31 needs S = 62 - 37 = 25 (all 40 atoms lie inside the crop box).  The exact value is known in
    closed form for an atom alone on a voxel: amp * exp(-(expo * d2)), a multiple of 2^-25 far below 2^53."""
    dm = device_map("box", gpu_ctx)
    rng = np.random.default_rng(2)
    lo, hi = model_cases.box_of("box")
    xyz = rng.uniform(lo, hi, size=(40, 3))
    radii = np.full(40, 1.0, dtype=np.float32)
    amp, expo = rng.uniform(0.5, 1.0, size=(40, 2)) * 2.0 ** 31, rng.uniform(1.0, 5.0, size=(40, 2))
    amp[7] = 2.0 ** 30                                              # A_max = 2^31 exactly
    amp[np.arange(40) != 7] *= 0.5
    want_s = model_checker.shift_rule(40, model_checker.a_max(amp))
    assert model_checker.a_max(amp) == 2.0 ** 31 and want_s == 25
    out = dm.modelDensity(xyz, amp, expo, radii)
    assert out.modelCounters["shift"] == want_s
    assert_density(out.density, model_checker.density(dm.header, xyz, amp, expo, radii, crs2xyz=where_of(dm)), "large amplitudes")


def _raw(dm, xyz, n_atoms, n_terms, amp, expo, radii):
    """pdbeda_model_density called directly: (status, the handle slot afterwards)."""
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    slot = ctypes.c_void_p(0x5eed)
    rc = dm._map._ctx._lib.pdbeda_model_density(dm._map._h, ptr(xyz), n_atoms, n_terms, ptr(amp), ptr(expo), ptr(radii), ctypes.byref(slot), None)
    return rc, slot.value


def test_refusals_leave_the_context_usable(gpu_ctx):
    from pdb_eda_amd import _native
    dm = device_map("box", gpu_ctx)
    xyz, amp, expo, radii = model_cases.scattered("box", n=8)
    good = (np.ascontiguousarray(xyz), np.ascontiguousarray(amp), np.ascontiguousarray(expo), np.ascontiguousarray(radii))

    def broken(which, index, value):
        arrays = [a.copy() for a in good]
        arrays[which].reshape(-1)[index] = value
        return arrays

    cases = {"n_terms 0": (good, 0), "n_terms 7": (good, 7)}
    for label, (which, value) in {"NaN coordinate": (0, np.nan), "infinite coordinate": (0, np.inf), "NaN amplitude": (1, np.nan), "infinite amplitude": (1, -np.inf),
                                  "NaN exponent": (2, np.nan), "infinite exponent": (2, np.inf), "negative exponent": (2, -1e-300), "zero radius": (3, 0.0),
                                  "negative radius": (3, -1.0), "infinite radius": (3, np.inf), "NaN radius": (3, np.nan),
                                  "radius of 2^29 grid steps": (3, 3.0e8),
                                  "amplitudes whose n_gridded * A_max is not finite": (1, 1.7e308)}.items():      # (finite itself; at least two of the 8 atoms are gridded)
        cases[label] = (broken(which, 5, value), 1)
    for label, (arrays, n_terms) in cases.items():
        rc, slot = _raw(dm, arrays[0], len(xyz), n_terms, arrays[1], arrays[2], arrays[3])
        assert rc == _native.PDBEDA_ERR_ARGUMENT and slot == 0x5eed, label
        assert dm._map._ctx._lib.pdbeda_last_error(dm._map._ctx._h), label
    rc, slot = _raw(dm, good[0], 2 ** 31, 1, good[1], good[2], good[3])          # (refused before anything is read)
    assert rc == _native.PDBEDA_ERR_ARGUMENT and slot == 0x5eed
    other = device_map("past", gpu_ctx)
    for floor in (np.nan,):
        rc = dm._map._ctx._lib.pdbeda_map_pair_moments(dm._map._h, dm._map._h, ctypes.c_float(floor), None, None)
        assert rc == _native.PDBEDA_ERR_ARGUMENT
    rc = dm._map._ctx._lib.pdbeda_map_pair_moments(dm._map._h, other._map._h, ctypes.c_float(0.0), None, None)
    assert rc == _native.PDBEDA_ERR_ARGUMENT          # maps of different shapes
    # the context still works, and a good call fills the slot
    out = dm.modelDensity(xyz, amp, expo, radii)
    assert_density(out.density, checker("scattered-8", dm, (xyz, amp, expo, radii)), "after the refusals")
    with pytest.raises(_native.PdbedaError):
        dm.modelDensity(xyz, amp, -expo, radii)


# ---- pdbeda_map_pair_moments ---------------------------------------------------------------------------------------------------------
def _pair_maps(gpu_ctx):
    """Two maps on the geometry whose stored box is larger than the unique one, with NaN and infinite voxels in either (and, outside the
    unique box, in both: never read)."""
    rng = np.random.default_rng(41)
    a = rng.normal(0.2, 1.0, size=(7, 9, 21)).astype(np.float32)
    b = (0.5 * a + rng.normal(0.0, 0.5, size=a.shape)).astype(np.float32)
    a[1, 2, 3], a[2, 2, 3], b[3, 3, 3], b[4, 4, 4], b[1, 2, 3] = np.nan, np.inf, np.nan, -np.inf, 1.0
    a[:, :, 17], b[:, :, 19] = np.nan, np.inf
    b[5, 5, 5] = b[0, 0, 0] = np.float32(0.25)          # the floor of the strict case: two voxels ON it
    return a, b, device_map("rep", gpu_ctx, a, "pair-a"), device_map("rep", gpu_ctx, b, "pair-b")


@pytest.mark.parametrize("floor", [None, -np.inf, 0.25, 1e30])
def test_pair_moments_against_checker(gpu_ctx, floor):
    a, b, da, db = _pair_maps(gpu_ctx)
    n_want, sums_want, scale = model_checker.pair_moments(da.header, a, b, floor)
    got = da.pairMoments(db, floor)
    n, sums = got[0], np.array(got[1:])
    err = np.abs(sums - sums_want)
    print("floor %s: n = %d, |sum - checker| = %s, bounds %s" % (floor, n, err.tolist(), (1e-9 * scale).tolist()))
    assert n == n_want and np.all(err <= 1e-9 * scale)
    box = 16 * 9 * 7
    if floor is None or floor == -np.inf:
        assert n == box - 4          # NaN / inf in a (2, one shared with nothing) and in b (2) inside the unique box
    elif floor == 0.25:
        strict = model_checker.pair_moments(da.header, a, b, np.nextafter(np.float32(0.25), np.float32(-1)))[0]
        assert 0 < n < box - 4 and strict == n + 2          # the two voxels ON the floor are out
    else:
        assert n == 0 and not sums.view(np.uint64).any()          # an empty selection: exactly +0.0
    again = da.pairMoments(db, floor)
    assert again[0] == n and np.array(again[1:]).tobytes() == sums.tobytes()
    fit = da.correlate(db, floor)
    cc, slope, offset = model_checker.correlation(n_want, sums_want)
    if n:
        assert abs(fit["cc"] - cc) <= 1e-9 and abs(fit["scale"] - slope) <= 1e-9 * abs(slope) and abs(fit["offset"] - offset) <= 1e-9 and fit["n"] == n
    else:
        assert fit["n"] == 0 and all(math.isnan(fit[k]) for k in ("cc", "scale", "offset"))


def test_correlation_of_a_constant_map_is_nan(gpu_ctx):
    flat = device_map("rep", gpu_ctx, np.full((7, 9, 21), 0.5, dtype=np.float32), "flat")
    _, _, da, _ = _pair_maps(gpu_ctx)
    fit = da.correlate(flat)
    assert fit["n"] > 0 and all(math.isnan(fit[k]) for k in ("cc", "scale", "offset"))
    assert math.isnan(flat.correlate(da)["cc"]) and flat.correlate(da)["scale"] == 0.0


# ---- electrons of one atom inside the box ------------------------------------------------------------------------------------------
def _one_atom_entry(gpu_ctx, coord, occupancy, bfactor):
    """A DensityAnalysis of ONE alanine CA (Z = 7 in the synthetic tables) in a 16 A cube at 0.5 A, identity symmetry only: the cell's
    translations put its images 16 A away, outside the symmetry list's 5 A margin, so the model is this atom alone."""
    from pdb_eda_amd import ccp4, densityAnalysis, structure, synthetic
    params = synthetic.synthetic_params()
    densityAnalysis.setGlobals(params)
    spec = synthetic.MapSpec(ncrs=(32, 32, 32), spacing=0.5)
    dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((32, 32, 32), dtype=np.float32))), "one", ctx=gpu_ctx)
    st = structure.Structure("one")
    residue = structure.Residue((" ", 1, " "), "ALA", structure.Chain("A", structure.Model(0, st)))
    structure.Atom("CA", np.asarray(coord, dtype=np.float32), occupancy, bfactor, "C", residue, 1)
    identity = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    pdb = structure.PDBEntry(structure.PDBHeader(pdbid="one", resolution=2.0, spaceGroup="P_1", rotationMats=[identity]))
    return densityAnalysis.DensityAnalysis("one", dens, None, st, pdb), params["full_atom_name_map_electrons"]["ALA_CA"]


@pytest.mark.parametrize("n_sigma", [None, 6.0], ids=["default", "6-sigma"])
def test_electrons_found_of_an_atom_inside_the_box(gpu_ctx, n_sigma):
    """``modelSummary`` of one atom (occupancy 0.75, B = 80: sigma 1.007 A) whose sphere lies inside the box: electrons found is electrons
    placed = occ * Z less the share beyond the cut-off, which the checker states in closed form.  The bound is the one
    tests/test_model_host.py derives, on this 0.5 A grid: the midpoint rule on a Gaussian of sigma / h = 2 is exact to exp(-2 pi^2 sigma^2 /
    h^2) = 1e-34 (1e-6 is allowed for it); what remains is the ragged edge of the sphere on the grid, bounded by the shell of one voxel
    diagonal around it, 4 pi R^2 * (sqrt 3 h) * rho(R - sqrt 3 h); and the voxels are float32, each within 2^-23 of the exact one.  At the
    default cut-off of 4 sigma that shell may hold 8 % of the atom; at 6 sigma 5e-5 of it, so a wrong amplitude, exponent or voxel volume
    anywhere below ``electrons_placed`` cannot pass."""
    from pdb_eda_amd import ccp4, densityAnalysis
    coord, occupancy, bfactor = [8.13, 8.21, 7.92], 0.75, 80.0
    an, z = _one_atom_entry(gpu_ctx, coord, occupancy, bfactor)
    sigmas = ccp4.MODEL_N_SIGMA if n_sigma is None else n_sigma
    before = densityAnalysis.modelSigmas
    try:
        densityAnalysis.modelSigmas = sigmas
        summary = an.modelSummary()
        model = an.modelDensityObj
    finally:
        densityAnalysis.modelSigmas = before
    assert len(an.symmetryAtomCoords) == 1
    placed = occupancy * z
    amp, expo, b_eff = ccp4.gaussianAtomTerms([z], [bfactor], [occupancy])
    big_r, h = float(ccp4.modelRadii(b_eff, sigmas)[0]), 0.5
    where = np.asarray(an.symmetryAtomCoords, dtype=np.float64)[0]
    lo, hi = np.zeros(3), np.full(3, 15.5)
    assert np.all(where - big_r > lo) and np.all(where + big_r < hi) and list(model.header.gridLength) == [h, h, h]
    want = placed * (1.0 - model_checker.truncated_fraction(sigmas))
    edge = 4 * math.pi * big_r ** 2 * (math.sqrt(3) * h) * float(amp[0]) * math.exp(-float(expo[0]) * (big_r - math.sqrt(3) * h) ** 2)
    bound = edge + 1e-6 + 2.0 ** -23 * placed
    found = summary["electrons_found"]
    print("cut-off %g sigma = %.4f A: electrons placed %.9f, found %.9f, placed less the truncation %.9f, |difference| %.3g, bound %.3g"
          % (sigmas, big_r, summary["electrons_placed"], found, want, abs(found - want), bound))
    assert summary["electrons_placed"] == placed
    assert abs(found - want) <= bound and found < placed
    # and the same figure from the checker's own exact voxels (every voxel within one float32 spacing: the sums within 2^-23)
    exact = model_checker.density(model.header, where[None, :], amp, expo, ccp4.modelRadii(b_eff, sigmas), chunk=4096)["exact"]
    exact_sum = math.fsum(exact.reshape(-1).tolist()) * model.header.unitVolume
    assert abs(found - exact_sum) <= 2.0 ** -23 * exact_sum


# ---- the analysis layer on the small synthetic entry --------------------------------------------------------------------------------
_entry = {}


def analysis(gpu_ctx, name="orth"):
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    if name not in _entry:
        z, spec, st, pdb, params = load_analysis_case(name)
        densityAnalysis.setGlobals(params)
        dens = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["dens"])), name, ctx=gpu_ctx)
        diff = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, z["diff"])), name, ctx=gpu_ctx)
        densityAnalysis._attachCutoffs(dens, diff)
        st.header = {"resolution": 2.0}
        _entry[name] =(densityAnalysis.DensityAnalysis(name, dens, diff, st, pdb), params)
    densityAnalysis.setGlobals(_entry[name][1])
    return _entry[name][0]


def _gather(header, grid, crs):
    """utils.getPointDensityFromCrs over a host grid: periodic wrap by the cell's interval, 0 where nothing is stored."""
    idx, ok = [], np.ones(len(crs), dtype=bool)
    for k in range(3):
        v, n, interval = crs[:, k].astype(np.int64), int(header.ncrs[k]), int(header.crsInterval[k])
        out = (v < 0) | (v >= n)
        v = np.where(out, np.mod(v, interval), v)
        ok &= (v >= 0) & (v < n)
        idx.append(np.clip(v, 0, n - 1))
    return np.where(ok, grid[idx[2], idx[1], idx[0]].astype(np.float64), 0.0)


def _restated(an, groups, radius, fit):
    """RSCC / RSR per group from the sphere voxels (voxels()) and the two downloaded maps, in plain numpy."""
    dens, model = an.densityObj, an.modelDensityObj
    xyz = np.array([c for g in groups for c in g], dtype=np.float64).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    bl = dens._map.sphere_blobs(xyz, np.full(len(xyz), radius, dtype=np.float32), off, 0.0)
    crs, voff = bl.voxels()
    group = np.repeat(bl.stats()["group"].astype(np.int64), np.diff(voff))
    rscc, rsr = np.full(len(groups), np.nan), np.full(len(groups), np.nan)
    for g in range(len(groups)):
        mine = np.unique(crs[group == g], axis=0)
        if len(mine) == 0:
            continue
        fo = _gather(dens.header, dens.density, mine)
        fc = _gather(dens.header, model.density, mine) * fit["scale"] + fit["offset"]
        rsr[g] = math.fsum(np.abs(fo - fc).tolist()) / math.fsum(np.abs(fo + fc).tolist())
        if len(mine) > 1:
            xm, ym = fo - fo.mean(), fc - fc.mean()
            rscc[g] = float(np.clip(np.dot(xm, ym) / math.sqrt(np.dot(xm, xm) * np.dot(ym, ym)), -1.0, 1.0))
    return rscc, rsr


def test_model_map_of_the_entry(gpu_ctx):
    from pdb_eda_amd import ccp4, densityAnalysis
    an = analysis(gpu_ctx)
    model = an.modelDensityObj
    grid = model.density
    assert grid.shape == an.densityObj.density.shape and grid.min() >= 0.0 and grid.max() > 0.0
    xyz, amp, expo, radii, placed = an._modelAtoms()
    assert len(xyz) > 0 and np.all(amp > 0)
    # at the voxel nearest to an atom the map holds at least the atom's own term (every term is positive) ...
    crs = an.densityObj._map.xyz2crs(xyz)
    inside = np.all((crs >= 0) & (crs < np.array(model.header.ncrs)), axis=1)
    assert inside.sum() >= 10
    where = an.densityObj._map.crs2xyz(crs[inside])
    d2 = ((where - xyz[inside]) ** 2).sum(axis=1)
    own = amp[inside] * np.exp(-expo[inside] * d2)
    assert np.all(np.sqrt(d2) < radii[inside])
    assert np.all(grid[crs[inside, 2], crs[inside, 1], crs[inside, 0]] >= own * (1 - 1e-6))
    # ... and the highest voxel of the map lies within a voxel's diagonal of an atom
    top = np.unravel_index(int(np.argmax(grid)), grid.shape)
    peak = an.densityObj._map.crs2xyz(np.array([[top[2], top[1], top[0]]], dtype=np.int32))[0]
    diagonal = math.sqrt(sum(float(v) ** 2 for v in model.header.gridLength))
    assert np.sqrt(((xyz - peak) ** 2).sum(axis=1)).min() <= diagonal
    # the summary: the electrons placed are those of the atoms the map was made from, the electrons found the box's voxels added up
    summary = an.modelSummary()
    cols = an.symmetryAtoms._cols
    rows = an.symmetryAtoms._idx
    table = densityAnalysis.fullAtomNameMapElectronsGlobal
    z = np.array([table.get(cols.pair_names[k], np.nan) for k in cols.pair_of_atom[rows]])
    keep = ~np.isnan(z) & (cols.occupancy[rows] != 0)
    assert keep.sum() == len(xyz) and summary["electrons_placed"] == placed == float(np.sum(z[keep] * cols.occupancy[rows][keep])) > 0
    box = model_checker.pair_moments(model.header, grid, grid)
    assert abs(summary["electrons_found"] - box[1][0] * model.header.unitVolume) <= 1e-9 * box[2][0] * model.header.unitVolume
    assert 0 < summary["electrons_found"] < summary["electrons_placed"]
    n, sums, _ = model_checker.pair_moments(model.header, an.densityObj.density, grid)
    cc, scale, offset = model_checker.correlation(n, sums)
    fit = an.modelCorrelation()
    print("entry: cc %.6f scale %.6f offset %.6f over %d voxels; electrons placed %.3f found %.3f" % (fit["cc"], fit["scale"], fit["offset"], fit["n"],
                                                                                                   summary["electrons_placed"], summary["electrons_found"]))
    assert fit["n"] == n and abs(fit["cc"] - cc) <= 1e-9 and abs(fit["scale"] - scale) <= 1e-9 * abs(scale) and abs(fit["offset"] - offset) <= 1e-9
    assert fit["cc"] > 0.5          # (the entry's 2Fo-Fc map was synthesised from these very atoms)
    assert summary["cc"] == fit["cc"] and summary["scale"] == fit["scale"] and summary["offset"] == fit["offset"] and summary["n"] == n
    part = an.modelCorrelation(floor=0.05)
    n2, sums2, _ = model_checker.pair_moments(model.header, an.densityObj.density, grid, 0.05)
    assert 0 < part["n"] == n2 < n and abs(part["cc"] - model_checker.correlation(n2, sums2)[0]) <= 1e-9
    # observed minus model: the combine formula, bit for bit, and a map the blob and peak code takes as it is
    difference = an.modelDifferenceObj
    formula = (an.densityObj.density.astype(np.float64) + (-fit["scale"]) * grid.astype(np.float64)).astype(np.float32)
    assert difference.density.tobytes() == formula.tobytes()
    cut = difference.meanDensity + 3 * difference.stdDensity
    blobs = difference.createFullBlobList(cut)
    assert blobs is not None and len(blobs) > 0 and len(difference.findPeaks(cut, blobs)) > 0


def test_model_correlation_tables(gpu_ctx):
    from pdb_eda_amd import singleStructure
    an = analysis(gpu_ctx)
    fit = an.modelCorrelation()
    atoms = list(an.biopdbObj.get_atoms())
    residues = list(an.biopdbObj.get_residues())
    for radius in (None, 1.1):
        used = an._metricsRadius() if radius is None else radius
        table = an.calculateAtomModelCorrelations(radius)
        assert len(table) == len(atoms) and all(len(row) == len(an.atomModelCorrelationHeader) for row in table)
        rscc, rsr = _restated(an, [[atom.coord] for atom in atoms], used, fit)
        for row, atom, cc, rr in zip(table, atoms, rscc, rsr):
            assert row[4] == atom.name and row[6] == atom.get_bfactor()
            assert (row[7] is None and cc != cc) or abs(row[7] - cc) <= 1e-9
            assert abs(row[8] - rr) <= 1e-9
        assert sum(row[7] is not None for row in table) >= len(atoms) // 2
        table = an.calculateResidueModelCorrelations(radius)
        assert len(table) == len(residues) and all(len(row) == len(an.residueModelCorrelationHeader) for row in table)
        rscc, rsr = _restated(an, [[atom.coord for atom in residue.child_list] for residue in residues], used, fit)
        for row, residue, cc, rr in zip(table, residues, rscc, rsr):
            assert row[3] == residue.resname and abs(row[5] - cc) <= 1e-9 and abs(row[6] - rr) <= 1e-9
    # the untouched tables still say what they said
    assert len(an.atomMetrics()) == len(an.asymmetryAtoms) and len(an.residueMetrics()) == len(residues)
    for level, count in (("atom", len(atoms)), ("residue", len(residues)), ("summary", 1)):
        header, rows = singleStructure.rows(an, "model", level)
        assert len(rows) == count and all(len(row) == len(header) for row in rows)
        assert header == {"atom": an.atomModelCorrelationHeader, "residue": an.residueModelCorrelationHeader,
                          "summary": ["cc", "scale", "offset", "n", "electrons_placed", "electrons_found"]}[level]
        assert singleStructure.dumps(header, rows)
    header, rows = singleStructure.rows(an, "model", "atom", includePdbid=True)
    assert header[0] == "pdbid" and rows[0][0] == an.pdbid
    with pytest.raises(ValueError):
        singleStructure.rows(an, "model", "domain")
