"""The crystal-contact entry points (pdbeda_coord_contacts, pdbeda_crystal_contacts, pdbeda_image_coords) at their grid and staging edges,
bit for bit against the numpy restatement (tests/contacts_checker.py) on the inputs of tests/contacts_cases.py; tests/test_contacts_host.py
proves on the CPU that every input reaches the corner it is named for.

Not covered: the grid-stride loops past grid_for's 2^20 blocks (k_image_select and its kin need 2.7e8 (candidate, atom) lanes for a second
trip; no CPU reference of that size stays within a few seconds)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import contacts_cases as cases
import contacts_checker as chk

pytestmark = pytest.mark.gpu

ERR_ARGUMENT, ERR_CAPACITY = -2, -4          # PDBEDA_ERR_ARGUMENT, PDBEDA_ERR_CAPACITY (include/pdbeda.h)
GUARD_I, GUARD_D = -7, -7.5


def assert_rows(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert got[1].tobytes() == np.ascontiguousarray(want[1]).tobytes(), what


# ---- 1. large results: the staging paths ----------------------------------------------------------------------------------------------------
def test_mixed_staging_index_through_the_block_distance_through_the_device(gpu_ctx):
    """300 000 queries: rows = min(cap, n_q) = 300 000.  The index column is 8 x 300 000 = 2 400 000 bytes <= 4 194 304 (the pinned block): the
    kernel writes it there.  The block then has 1 794 304 bytes left, fewer than the distance column's 2 400 000: that column is written on
    the device and copied.  Beside 16 n_q + 64 bytes of results the block has no room for the inputs (7.2 MB + 5.5 MB + 4 x 131^3 bytes of
    zeroed cell counts), which are copied item by item.  8 (n_q + n_p) > 2^22: the grid has the cap's upper bound and coarsens twice."""
    q, p, cutoff = cases.coord_case("mixed")
    want = cases.expected_coord("mixed")
    got = gpu_ctx.coord_contacts(q, p, cutoff)
    print("mixed: %d rows" % len(got[0]))
    assert_rows(got, want, "mixed")


def test_device_staging_for_both_columns(gpu_ctx):
    """600 000 queries: each column is 4 800 000 bytes > 4 194 304, so both are written on the device and copied; the count alone uses the block."""
    q, p, cutoff = cases.coord_case("device")
    want = cases.expected_coord("device")
    got = gpu_ctx.coord_contacts(q, p, cutoff)
    print("device: %d rows" % len(got[0]))
    assert_rows(got, want, "device")


def test_keep_flags_of_a_million_candidates(gpu_ctx):
    """103^3 - 1 = 1 092 726 candidates: the keep flags are 4 x 1 092 726 = 4 370 904 bytes > 4 194 304, so k_image_count cannot hand them over
    through the block (r_keep is null) and they are copied from the device; the inputs (17.5 MB of candidates) are copied item by item."""
    query, poly, rot, ortho, cand, cutoff = cases.many_candidates()
    keep = chk.kept_images_diag(np.diag(ortho), poly, cand, cutoff)
    want = chk.coord_contacts(query, chk.neighbours(rot, ortho, poly, cand[keep]), cutoff)
    kept, idx, dist = gpu_ctx.crystal_contacts(query, poly, rot, ortho, cand, cutoff)
    assert keep.sum() == 8 and np.array_equal(kept, keep)
    assert_rows((idx, dist), want, "many candidates")


def test_image_coords_beyond_the_block(gpu_ctx):
    """40 images x 5 000 atoms x 24 bytes = 4 800 000 > 4 194 304: k_image_emit writes to the device and the list is copied."""
    poly, rot, ortho, cand = cases.many_images()
    got = gpu_ctx.image_coords(poly, rot, ortho, cand)
    assert got.tobytes() == chk.neighbours(rot, ortho, poly, cand).tobytes()


# ---- the ordinary calls that cases 2, 3 and 9 repeat under other conditions -----------------------------------------------------------------------
_default = {}


def default_results(ctx):
    """(coord rows, crystal (kept, index, distance), image coordinates of the kept images) on the default context, checked once."""
    if not _default:
        q, p, cutoff = cases.coord_case("ordinary")
        query, poly, rot, ortho, cand, ccut = cases.crystal_case("ordinary")
        coord = ctx.coord_contacts(q, p, cutoff)
        crystal = ctx.crystal_contacts(query, poly, rot, ortho, cand, ccut)
        images = ctx.image_coords(poly, rot, ortho, cand[crystal[0]])
        assert_rows(coord, cases.expected_coord("ordinary"), "coord")
        want = cases.expected_crystal("ordinary")
        assert np.array_equal(crystal[0], want[0])
        assert_rows(crystal[1:], want[1:], "crystal")
        assert images.tobytes() == chk.neighbours(rot, ortho, poly, cand[want[0]]).tobytes()
        _default.update(coord=coord, crystal=crystal, images=images)
    return _default


def same_as_default(ctx, coord, crystal, images, what):
    d = default_results(ctx)
    for got, want in ((coord[0], d["coord"][0]), (coord[1], d["coord"][1]), (crystal[0], d["crystal"][0]), (crystal[1], d["crystal"][1]),
                      (crystal[2], d["crystal"][2]), (images, d["images"])):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


# ---- 2. PDBEDA_COPY_KERNELS=0 -----------------------------------------------------------------------------------------------------------------
SWITCH_WORKER = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
from pdb_eda_amd import _native
import contacts_cases as cases
ctx = _native.Context(0)
q, p, cutoff = cases.coord_case("ordinary")
query, poly, rot, ortho, cand, ccut = cases.crystal_case("ordinary")
ci, cd = ctx.coord_contacts(q, p, cutoff)
kept, xi, xd = ctx.crystal_contacts(query, poly, rot, ortho, cand, ccut)
images = ctx.image_coords(poly, rot, ortho, cand[kept])
np.savez(%(out)r, ci=ci, cd=cd, kept=kept, xi=xi, xd=xd, images=images)
ctx.close()
'''


def test_contacts_without_copy_kernels(gpu_ctx, tmp_path):
    """PDBEDA_COPY_KERNELS=0 in a fresh process: pinned_out hands out nothing, so every result of the three calls (rows, count, keep flags,
    neighbour total, image list) is written on the device and copied by the runtime.  The same bytes as the default mode and the checker."""
    script, out = tmp_path / "worker.py", tmp_path / "rows.npz"
    script.write_text(SWITCH_WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "out": str(out)})
    proc = subprocess.run([sys.executable, str(script)], env=dict(os.environ, PDBEDA_COPY_KERNELS="0"), capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stderr[-3000:]
    z = np.load(str(out))
    same_as_default(gpu_ctx, (z["ci"], z["cd"]), (z["kept"], z["xi"], z["xd"]), z["images"], "without copy kernels")


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------------------------
def _raw_coord(ctx, q, p, cutoff, cap, size):
    from pdb_eda_amd._native import _ptr
    idx, dist, n = np.full(size, GUARD_I, dtype=np.int64), np.full(size, GUARD_D), C.c_int64(-1)
    rc = ctx._lib.pdbeda_coord_contacts(ctx._h, _ptr(q), len(q), _ptr(p), len(p), C.c_double(cutoff), _ptr(idx), _ptr(dist), cap, C.byref(n))
    return rc, n.value, idx, dist, None


def _raw_crystal(ctx, query, poly, rot, ortho, cand, cutoff, cap, size):
    from pdb_eda_amd._native import _ptr
    rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 12)
    ortho = np.ascontiguousarray(ortho, dtype=np.float64).reshape(9)
    idx, dist, n = np.full(size, GUARD_I, dtype=np.int64), np.full(size, GUARD_D), C.c_int64(-1)
    kept = np.full(len(cand), 9, dtype=np.uint8)
    rc = ctx._lib.pdbeda_crystal_contacts(ctx._h, _ptr(query), len(query), _ptr(poly), len(poly), _ptr(rot), len(rot), _ptr(ortho), _ptr(cand), len(cand),
                                          C.c_double(cutoff), _ptr(kept), _ptr(idx), _ptr(dist), cap, C.byref(n))
    return rc, n.value, idx, dist, kept


@pytest.mark.parametrize("entry", ["coord", "crystal"])
def test_capacity_is_reported_and_respected(gpu_ctx, entry):
    """cap below the row count R: PDBEDA_ERR_CAPACITY, n_out = R, "capacity" in the message, nothing written at or past cap (the arrays hold
    R guard values; below cap the header promises nothing).  cap = R: the checker's rows.  The context answers the next call as before."""
    if entry == "coord":
        args = cases.coord_case("ordinary")
        want = cases.expected_coord("ordinary")
        call = lambda cap, size: _raw_coord(gpu_ctx, *args, cap, size)
    else:
        args = cases.crystal_case("ordinary")
        want_keep, *want = cases.expected_crystal("ordinary")
        call = lambda cap, size: _raw_crystal(gpu_ctx, *args, cap, size)
    rows = len(want[0])
    assert 100 <= rows < len(args[0])
    for cap in (0, 1, rows - 1):
        rc, n, idx, dist, kept = call(cap, rows)
        print("%s: cap %d of %d: status %d, n_out %d" % (entry, cap, rows, rc, n))
        assert rc == ERR_CAPACITY and n == rows
        assert b"capacity" in gpu_ctx._lib.pdbeda_last_error(gpu_ctx._h)
        assert np.all(idx[cap:] == GUARD_I) and np.all(dist[cap:] == GUARD_D)
        if kept is not None:
            assert np.array_equal(kept.astype(bool), want_keep) and kept.max() == 1
    rc, n, idx, dist, kept = call(rows, rows + 3)
    assert rc == 0 and n == rows
    assert_rows((idx[:rows], dist[:rows]), want, entry)
    assert np.all(idx[rows:] == GUARD_I) and np.all(dist[rows:] == GUARD_D)
    again = gpu_ctx.coord_contacts(*args) if entry == "coord" else gpu_ctx.crystal_contacts(*args)[1:]
    assert_rows(again, want, entry + " after the refusals")


# ---- 4. degenerate sets -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.degenerate_coord()))
def test_degenerate_coord(gpu_ctx, name):
    q, p, cutoff = cases.coord_case("degenerate", name)
    got = gpu_ctx.coord_contacts(q, p, cutoff)
    assert_rows(got, cases.expected_coord("degenerate", name), name)
    if name == "one on one":
        assert got[0].tolist() == [0] and got[1].tolist() == [0.0]
    if name.startswith("at cutoff"):
        assert got[1].tolist() == [5.0]


@pytest.mark.parametrize("name", sorted(cases.degenerate_crystal()))
def test_degenerate_polymer(gpu_ctx, name):
    query, poly, rot, ortho, cand, cutoff = cases.crystal_case("degenerate", name)
    want = cases.expected_crystal("degenerate", name)
    kept, idx, dist = gpu_ctx.crystal_contacts(query, poly, rot, ortho, cand, cutoff)
    assert np.array_equal(kept, want[0]), name
    assert_rows((idx, dist), want[1:], name)
    assert gpu_ctx.image_coords(poly, rot, ortho, cand[kept]).tobytes() == chk.neighbours(rot, ortho, poly, cand[want[0]]).tobytes()


# ---- 5. grid corners --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.grid_corners()))
def test_grid_corners(gpu_ctx, name):
    q, p, cutoff = cases.coord_case("corners", name)
    want = cases.expected_coord("corners", name)
    assert len(want[0]) >= 200
    assert_rows(gpu_ctx.coord_contacts(q, p, cutoff), want, name)


# ---- 6. exact-boundary images ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["identity", "twofold"])
def test_images_at_exactly_the_cutoff(gpu_ctx, case):
    """An image atom exactly 5.0 from an atom of the asymmetric unit keeps its image at cutoff 5.0 (<=) and gives a row of distance 5.0; at the
    next double below 5.0 no image is kept and there is no row."""
    poly, rot, ortho, cand = cases.boundary_identity() if case == "identity" else cases.boundary_twofold()
    want_keep, want_idx, want_dist = chk.crystal_contacts(poly, rot, ortho, poly, cand, 5.0)
    images = [(0, -1, 0, 0), (0, 1, 0, 0)] + ([(1, -1, 0, 0), (1, 0, 0, 0)] if case == "twofold" else [])
    assert [tuple(k) for k in cand[want_keep].tolist()] == images and want_dist.tolist() == [5.0] * len(images)
    kept, idx, dist = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    assert np.array_equal(kept, want_keep)
    assert_rows((idx, dist), (want_idx, want_dist), case)
    kept, idx, dist = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, cases.BELOW_FIVE)
    assert not kept.any() and len(idx) == 0 and len(dist) == 0


# ---- 7. shifts ----------------------------------------------------------------------------------------------------------------------------------
def test_largest_shift_is_accepted_and_one_more_refused(gpu_ctx):
    from pdb_eda_amd import _native
    poly, rot, ortho, _ = cases.boundary_identity()
    cand = np.array([[0, cases.MAX_SHIFT, 0, 0]], dtype=np.int32)
    kept, idx, dist = gpu_ctx.crystal_contacts(poly, poly, rot, ortho, cand, 5.0)
    assert kept.tolist() == [False] and len(idx) == 0
    got = gpu_ctx.image_coords(poly, rot, ortho, cand)
    assert got.tobytes() == chk.neighbours(rot, ortho, poly, cand).tobytes() and got[:, 0].min() > 4.19e7
    gpu_ctx.profile_begin()
    for bad in ([[0, cases.MAX_SHIFT + 1, 0, 0]], [[0, 0, 0, -(cases.MAX_SHIFT + 1)]]):
        bad = np.array(bad, dtype=np.int32)
        for call in (lambda: gpu_ctx.crystal_contacts(poly, poly, rot, ortho, bad, 5.0), lambda: gpu_ctx.image_coords(poly, rot, ortho, bad)):
            with pytest.raises(_native.PdbedaError) as e:
                call()
            assert e.value.code == ERR_ARGUMENT and "shift" in str(e.value)
    launched = gpu_ctx.profile_end()
    assert sum(calls for calls, _ in launched.values()) == 0, launched          # (refused before any launch)


# ---- 7b. extents that overflow fp64 ---------------------------------------------------------------------------------------------------------------
def _within(seconds, call):
    """call() on a thread of its own (the library releases the GIL): its result or exception, or a failure when it has not returned in time."""
    import threading
    box = {}

    def work():
        try:
            box["value"] = call()
        except BaseException as e:      # (handed to the test's thread)
            box["error"] = e

    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(seconds)
    assert not t.is_alive(), "the call has not returned after %g s" % seconds
    if "error" in box:
        raise box["error"]
    return box["value"]


@pytest.mark.parametrize("entry", ["coord", "crystal"])
def test_an_overflowing_extent_is_refused_not_searched_for_ever(gpu_ctx, entry):
    """Two query points at +-1e308 among ordinary ones: every coordinate is finite, the extent of their box is not.  No cell grid can be laid
    over it (make_cell_grid once enlarged its edge for ever): PDBEDA_ERR_ARGUMENT that names the extent, before anything is staged or
    launched, and the context answers the next ordinary call as before."""
    from pdb_eda_amd import _native
    if entry == "coord":
        args = cases.coord_case("ordinary")
        want = cases.expected_coord("ordinary")
        call = lambda q: gpu_ctx.coord_contacts(q, *args[1:])
    else:
        args = cases.crystal_case("ordinary")
        want = cases.expected_crystal("ordinary")[1:]
        call = lambda q: gpu_ctx.crystal_contacts(q, *args[1:])[1:]
    far = np.concatenate([[[1e308, 0.0, 0.0], [-1e308, 0.0, 0.0]], args[0][:6]])
    assert np.all(np.isfinite(far))
    gpu_ctx.profile_begin()
    with pytest.raises(_native.PdbedaError) as e:
        _within(20.0, lambda: call(far))
    launched = gpu_ctx.profile_end()
    print("%s: %s" % (entry, e.value))
    assert e.value.code == ERR_ARGUMENT and "extent" in str(e.value) and "overflows" in str(e.value) and "along x" in str(e.value)
    assert sum(calls for calls, _ in launched.values()) == 0, launched
    assert_rows(_within(60.0, lambda: call(args[0])), want, entry + " after the refusal")


# ---- 8. branches --------------------------------------------------------------------------------------------------------------------------------
def test_branches_without_rows(gpu_ctx):
    query, poly, rot, ortho, cand, cutoff = cases.crystal_case("ordinary")
    want_keep = cases.expected_crystal("ordinary")[0]
    none = np.zeros((0, 3))
    # no query: the keep flags alone
    kept, idx, dist = gpu_ctx.crystal_contacts(none, poly, rot, ortho, cand, cutoff)
    assert want_keep.any() and np.array_equal(kept, want_keep) and len(idx) == 0 and len(dist) == 0
    # queries far from every neighbour: images are kept, every image atom is cropped from the queries' grid (the neighbour total is 0)
    far = cases.crystal_case("far")[0]
    kept, idx, dist = gpu_ctx.crystal_contacts(far, poly, rot, ortho, cand, cutoff)
    assert np.array_equal(kept, cases.expected_crystal("far")[0]) and kept.any() and len(idx) == 0 and len(dist) == 0
    # no candidate; no polymer atom
    kept, idx, dist = gpu_ctx.crystal_contacts(query, poly, rot, ortho, np.zeros((0, 4), dtype=np.int32), cutoff)
    assert len(kept) == 0 and len(idx) == 0 and len(dist) == 0
    kept, idx, dist = gpu_ctx.crystal_contacts(query, none, rot, ortho, cand, cutoff)
    assert len(kept) == len(cand) and not kept.any() and len(idx) == 0 and len(dist) == 0
    assert gpu_ctx.image_coords(none, rot, ortho, cand).shape == (0, 3) and gpu_ctx.image_coords(poly, rot, ortho, cand[:0]).shape == (0, 3)
    # and the ordinary call after them
    kept, idx, dist = gpu_ctx.crystal_contacts(query, poly, rot, ortho, cand, cutoff)
    assert np.array_equal(kept, want_keep)
    assert_rows((idx, dist), cases.expected_crystal("ordinary")[1:], "after the empty calls")


# ---- 9. poisoned arenas -----------------------------------------------------------------------------------------------------------------------
def test_contacts_on_poisoned_arenas(gpu_ctx, monkeypatch):
    """On a context whose arenas are handed out filled with 0xFF (PDBEDA_DEBUG_POISON=1), twice (the second pass runs in the arenas the first
    gave back): the same bytes as the default context and the checker, so no contacts kernel trusts recycled memory -- cell counts, keep flags,
    cursors, the rows' count."""
    from pdb_eda_amd import _native
    default_results(gpu_ctx)
    q, p, cutoff = cases.coord_case("ordinary")
    query, poly, rot, ortho, cand, ccut = cases.crystal_case("ordinary")
    monkeypatch.setenv("PDBEDA_DEBUG_POISON", "1")
    ctx = _native.Context(0)
    try:
        for rep in range(2):
            coord = ctx.coord_contacts(q, p, cutoff)
            crystal = ctx.crystal_contacts(query, poly, rot, ortho, cand, ccut)
            images = ctx.image_coords(poly, rot, ortho, cand[crystal[0]])
            same_as_default(gpu_ctx, coord, crystal, images, "poisoned arenas, pass %d" % rep)
    finally:
        ctx.close()
