"""The spread without a GPU: the numpy restatement (tests/spread_checker.py) against scipy's morphology on a wrap-padded periodic map, the host
helpers of ccp4 (spreadTable, softEdgeValues, maskRadii) and of the bulk-solvent fit on made-up shell sums with a known answer, and THE GUARD:
every case the GPU test compares -- except "none" and "all" -- leaves at least 5 % of the map reached and at least 5 % unreached, asserted on
the checker's answer alone, so that no case can pass by being trivially full or empty."""
import numpy as np
import pytest
from scipy import ndimage

from pdb_eda_amd import ccp4, densityAnalysis

import spread_cases as cases
import spread_checker as checker


# ---- 1. the checker against scipy ----------------------------------------------------------------------------------------------------------
def test_checker_agrees_with_scipy_on_the_periodic_box():
    """Dilation and the bounded Euclidean distance of the periodic `box` at 2.0 A: scipy on the array padded by its own copies (np.pad, wrap),
    cropped back.  Sets identical; distances equal to the last bit of float32 (both are sqrt of one integer sum of squares times 0.25)."""
    h = cases.header_of("box")
    offsets, distance = ccp4.spreadTable(h, 2.0)
    x, threshold, below = cases.grid("noise30", "box")
    seed = checker.seeds_of(x, threshold, below)
    assert 0 < seed.sum() < seed.size
    t = checker.ranks(x, offsets, cases.intervals_of("box"), threshold, below)
    pad = int(np.abs(offsets).max())
    wide = np.pad(seed, pad, mode="wrap")
    edt = ndimage.distance_transform_edt(~wide, sampling=0.5)[pad:-pad, pad:-pad, pad:-pad]
    reached = t < len(offsets)
    assert np.array_equal(reached, edt <= 2.0 + 1e-9)
    ball = np.zeros((2 * pad + 1,) * 3, dtype=bool)
    ball[offsets[:, 2] + pad, offsets[:, 1] + pad, offsets[:, 0] + pad] = True
    assert np.array_equal(reached, ndimage.binary_dilation(wide, structure=ball)[pad:-pad, pad:-pad, pad:-pad])
    got = np.append(distance, np.inf)[t]
    assert np.array_equal(got[reached], edt[reached]) or float(np.abs(got[reached] - edt[reached]).max()) == 0.0


def test_checker_takes_the_first_entry_not_the_nearest():
    """The rank is the table's order, whatever it means: a reversed ball answers with the farthest seed."""
    x, threshold, _ = cases.grid("pair", "box")
    offsets = cases.table("ball25", "box")[0]
    iv = cases.intervals_of("box")
    fwd, rev = checker.ranks(x, offsets, iv, threshold), checker.ranks(x, offsets[::-1], iv, threshold)
    assert np.array_equal(fwd < len(offsets), rev < len(offsets))
    both = fwd < len(offsets)
    assert (fwd[both] + rev[both] <= len(offsets) - 1).all() and (fwd[both] + rev[both] < len(offsets) - 1).any()
    assert np.array_equal(checker.ranks(x, np.concatenate([offsets, offsets[3:4]]), iv, threshold)[both], fwd[both])      # a duplicate: the smallest t wins


# ---- 2. host helpers -----------------------------------------------------------------------------------------------------------------------
def test_spread_table_is_neighbour_offsets_under_the_limits():
    h = cases.header_of("box")
    offsets, distance = ccp4.spreadTable(h, 2.5)
    ref = ccp4.neighbourOffsets(h, 2.5)
    assert np.array_equal(offsets, ref[0]) and np.array_equal(distance, ref[1])
    assert tuple(offsets[0]) == (0, 0, 0) and (np.diff(distance) >= 0).all() and int(np.abs(offsets).max()) == 5
    with pytest.raises(ValueError):
        ccp4.spreadTable(h, 16.5)                                     # 33 steps
    with pytest.raises(ValueError):
        ccp4.spreadTable(h, 8.5)                                      # inside +-32, more than 16384 offsets
    offsets, _, radius = cases.largest_ball()
    assert len(offsets) <= cases.MAX_OFFSETS and int(np.abs(offsets).max()) <= cases.MAX_REACH
    with pytest.raises(ValueError):
        ccp4.spreadTable(cases.header_of("big"), radius + 0.05)
    line = ccp4.spreadTable(cases.header_of("line"), 0.0)[0]
    assert line.shape == (1, 3)


def test_soft_edge_values():
    d = np.array([0.0, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5])
    v = ccp4.softEdgeValues(d, 1.0, 2.0)
    assert v.dtype == np.float32 and len(v) == len(d) + 1
    want = [1.0, 1.0, 0.5 * (1 + np.cos(np.pi * 0.25)), 0.5, 0.5 * (1 + np.cos(np.pi * 0.75)), 0.0, 0.0, 0.0]
    assert np.array_equal(v, np.array(want, dtype=np.float32))
    assert np.array_equal(ccp4.softEdgeValues(d, 2.0, 0.0), np.array([1, 1, 1, 1, 0, 0, 0, 0], dtype=np.float32))
    assert (np.diff(ccp4.softEdgeValues(np.linspace(0, 4, 101), 1.0, 2.0)) <= 0).all()
    with pytest.raises(ValueError):
        ccp4.softEdgeValues(d, -1.0, 1.0)


def test_mask_radii():
    r = ccp4.maskRadii(["C", " n", "Xx", "se", ""])
    assert list(r) == [ccp4.MASK_VDW["C"], ccp4.MASK_VDW["N"], 1.8, ccp4.MASK_VDW["SE"], 1.8] and ccp4.MASK_VDW_DEFAULT == 1.8


def _shell_sums(rng, n_shells, a, b, noise=0.0):
    """Per shell the Hermitian sums of a made-up (Fc, S): |Fc|^2, |S|^2, Re Fc S*, and those of Fo = a Fc + b S (+ an orthogonal rest)."""
    cc = rng.uniform(1.0, 5.0, n_shells)
    ss = rng.uniform(0.5, 2.0, n_shells)
    cs = rng.uniform(-0.6, 0.6, n_shells) * np.sqrt(cc * ss)
    oc = a * cc + b * cs
    os_ = a * cs + b * ss
    oo = a * a * cc + 2 * a * b * cs + b * b * ss + noise
    return oo, cc, ss, oc, os_, cs


def test_flat_solvent_fit_recovers_a_known_answer():
    """Fo = 1.7 Fc - 0.35 S exactly: the normal equations give the two coefficients and a residual of 0; with a rest orthogonal to both the
    coefficients stay and the residual is the rest."""
    rng = np.random.default_rng(1)
    oo, cc, ss, oc, os_, cs = _shell_sums(rng, 12, 1.7, -0.35)
    fit = densityAnalysis.flatSolventFit(oo, cc, ss, oc, os_, cs)
    assert abs(fit["scale"] - 1.7) < 1e-12 and abs(fit["b"] + 0.35) < 1e-12 and abs(fit["kSol"] + 0.35 / 1.7) < 1e-12
    assert abs(fit["residual"]) < 1e-10 * oo.sum()
    assert np.allclose(fit["fscAfter"], 1.0, atol=1e-12) and (fit["fscBefore"] < 1.0).all()
    oo2 = oo + 0.25
    fit2 = densityAnalysis.flatSolventFit(oo2, cc, ss, oc, os_, cs)
    assert abs(fit2["scale"] - 1.7) < 1e-12 and abs(fit2["residual"] - 0.25 * 12) < 1e-9
    flat = densityAnalysis.flatSolventFit(oo, cc, np.zeros(12), oc, np.zeros(12), np.zeros(12))      # no mask spectrum: a scale alone
    assert flat["b"] == 0.0 and abs(flat["scale"] - oc.sum() / cc.sum()) < 1e-15


# ---- 3. the guard ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.compared_cases(), ids=lambda c: c[0])
def test_guard_every_compared_case_shows_something(case):
    tag, geometry, table, seeds, _, _ = case
    offsets = cases.table(table, geometry)[0]
    x, threshold, below = cases.grid(seeds, geometry)
    t = checker.ranks(x, offsets, cases.intervals_of(geometry), threshold, below)
    reached = float((t < len(offsets)).mean())
    if seeds == "none":
        assert reached == 0.0
    elif seeds == "all":
        assert reached == 1.0
    else:
        assert 0.05 <= reached <= 0.95, "%s reaches %.1f %% of the map" % (tag, 100 * reached)
        if len(offsets) > 1 and table != "needle_up":
            assert len(np.unique(t)) > 2, "more than one rank must occur"
