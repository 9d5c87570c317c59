"""The atom-gradient yardstick without a GPU: the ABI of pdbeda_atom_moments, the chain rule of ccp4.gaussianAtomGradients against central
differences of an fp64 restatement of sum_v w rho (and of the profiled least-squares target, scale and offset re-fitted at every point: the
envelope argument of DensityMatrix.refineGaussianAtoms), the fold of image gradients through a rotation, the clamp below minB, the step
rule on a one-atom case, and the conditioning of every case tests/test_gpu_gradient.py runs.

The finite-difference bound calibrates itself: |analytic - FD(h/2)| <= |FD(h) - FD(h/2)| + the rounding of the sums.  A central difference
errs by c h^2 + O(h^4), so FD(h) - FD(h/2) is three quarters of c h^2 while FD(h/2) is off by one quarter of it; a sum of terms t is
known to sum|t| 2^-50 at the worst (fsum is exact; the terms carry a few roundings each), and the quotient divides that by the step.  No
tolerance is picked by hand.  The comparison is made only where the pair set is the same at theta - h, theta and theta + h: asserted."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import gradient_cases as cases
import gradient_checker as checker


def test_abi_has_the_entry_point():
    import __graft_entry__ as entry
    entry.build()
    from pdb_eda_amd import _native, ccp4, densityAnalysis as da, singleStructure
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdbeda.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_native.LIB_PATH)
    assert "pdbeda_atom_moments" in _native.EXPORTED_SYMBOLS and hasattr(handle, "pdbeda_atom_moments") and re.search(r"\bpdbeda_atom_moments\s*\(", text)
    assert "#define PDBEDA_MOMENTS_UNIQUE_BOX 1u" in text and _native.MOMENTS_UNIQUE_BOX == 1
    assert hasattr(_native.DeviceMap, "atom_moments")
    assert all(hasattr(ccp4.DensityMatrix, name) for name in ("atomMoments", "refineGaussianAtoms"))
    assert all(hasattr(ccp4, name) for name in ("gaussianAtomGradients", "gaussianAtomCurvatures", "foldImageGradients", "gaussNewtonStep"))
    assert all(hasattr(da.DensityAnalysis, name) for name in ("calculateAtomGradients", "refineAtoms", "refineSummary"))
    assert "refine" in singleStructure.MODES and all(("refine", level) in singleStructure.TABLES for level in ("atom", "summary"))
    plan = open(os.path.join(ROOT, "pdb_eda_amd", "csrc", "pdbeda_gradplan.h")).read()
    assert "#include <hip" not in plan and "__global__" not in plan and "__device__" not in plan and "pdbeda_device.h" not in plan      # the plan is HIP-free
    assert int(re.search(r"GP_MAX_TERMS\s*=\s*(\d+)", plan).group(1)) == checker.MAX_TERMS and "#define PDBEDA_MODEL_MAX_TERMS 6" in text
    assert float.fromhex(re.search(r"GP_PAD\s*=\s*(0x[0-9a-fp.+-]+)", plan).group(1)) == checker.PAD


@pytest.mark.parametrize("case", cases.cases(), ids=[c[0] for c in cases.cases()])
def test_conditioning_of_the_gpu_cases(case):
    """No pair within 1e-9 of its sphere (membership must not hinge on an ulp of crs2xyz or of the distance), and the case is not vacuous."""
    tag, name, kind, unique, xyz, expo, radii = case
    got = checker.moments(cases.header_of(name), cases.weight(name, kind), xyz, expo, radii, unique=unique, key=name)
    print("%s: nearest approach to a sphere %.3g, pairs %d, E_max %.3g" % (tag, got["nearest_sphere"], int(got["nVoxels"].sum()), got["e_max"]))
    assert got["on_sphere"] == 0 and got["nearest_sphere"] > 1e-9
    assert got["nVoxels"].sum() > 500 and got["e_max"] <= 6.5


# ---- the chain rule against central differences ------------------------------------------------------------------------------------------------
H_XYZ, H_B, H_OCC = 2e-5, 1e-2, 1e-3          # (a step along x small enough that no voxel crosses a sphere: asserted where it is used)


class Scene(object):
    """A few one-Gaussian atoms on ``box`` with a random fp64 weight map, radii held FIXED (the sums differentiate at a fixed pair set)."""

    def __init__(self, name="box", seed=5, n=4):
        from pdb_eda_amd import ccp4
        self.ccp4 = ccp4
        rng = np.random.default_rng(seed)
        self.name = name
        self.header = cases.header_of(name)
        lo, hi = cases.box_of(name)
        mid, span = 0.5 * (lo + hi), hi - lo
        self.xyz = mid + rng.uniform(-0.3, 0.3, size=(n, 3)) * span
        self.z = rng.choice([6.0, 7.0, 8.0], size=n)
        self.b = rng.uniform(15.0, 40.0, size=n)
        self.occ = rng.uniform(0.5, 1.0, size=n)
        self.radii = ccp4.modelRadii(ccp4.gaussianAtomTerms(self.z, self.b, self.occ)[2], 2.5)
        shape = (int(self.header.ncrs[2]), int(self.header.ncrs[1]), int(self.header.ncrs[0]))
        self.w = rng.uniform(-1.0, 1.0, size=shape)
        self.crs = checker.domain_crs(self.header, True)
        self.where = checker.voxel_xyz(self.header, self.crs, (name, True, False))

    def pairs(self, xyz):
        """The pair set: a boolean (voxels, atoms) array."""
        d = self.where[:, None, :] - np.asarray(xyz)[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        return np.sqrt(d2) <= self.radii.astype(np.float64)[None, :], d2

    def density(self, xyz, b, occ):
        """The fp64 model on the voxels of the unique box ((voxels,) and the (voxels, atoms) terms)."""
        amp, expo, _ = self.ccp4.gaussianAtomTerms(self.z, b, occ)
        inside, d2 = self.pairs(xyz)
        terms = np.where(inside, amp[None, :] * np.exp(-(expo[None, :] * d2)), 0.0)
        return np.array([math.fsum(row.tolist()) for row in terms]), terms

    def weights(self, w):
        return w[self.crs[:, 2], self.crs[:, 1], self.crs[:, 0]]

    def weighted_sum(self, xyz, b, occ):
        """(F, sum|t|) of F = sum_v w rho."""
        t = self.weights(self.w)[:, None] * self.density(xyz, b, occ)[1]
        return math.fsum(t.reshape(-1).tolist()), math.fsum(np.abs(t).reshape(-1).tolist())

    def target(self, obs, xyz, b, occ):
        """(T, s, o, residual (voxels,), what T's roundings are relative to) with s and o re-fitted: the profiled target.  A residual is known to a few
        ulps of |obs| + |s calc| + |o|, so T to sum |res| (|obs| + |s calc| + |o|) + T; the roundings of s and o themselves do not enter to first order
        (T is stationary in them)."""
        calc = self.density(xyz, b, occ)[0]
        n = len(calc)
        sa, sb = math.fsum(obs.tolist()), math.fsum(calc.tolist())
        va = math.fsum(((obs - sa / n) ** 2).tolist())
        vb = math.fsum(((calc - sb / n) ** 2).tolist())
        cov = math.fsum(((obs - sa / n) * (calc - sb / n)).tolist())
        s = cov / vb
        o = (sa - s * sb) / n
        res = obs - s * calc - o
        t = 0.5 * math.fsum((res * res).tolist())
        return t, s, o, res, t + math.fsum((np.abs(res) * (np.abs(obs) + np.abs(s * calc) + abs(o))).tolist())

    def analytic(self, w_full, xyz, b, occ):
        amp, expo, _ = self.ccp4.gaussianAtomTerms(self.z, b, occ)
        got = checker.moments(self.header, w_full, xyz, expo, self.radii, unique=True, key=self.name)
        return self.ccp4.gaussianAtomGradients(got["exact"], self.z, b, occ), got

    def moved(self, which, a, k, h):
        xyz, b, occ = self.xyz.copy(), self.b.copy(), self.occ.copy()
        if which == "xyz":
            xyz[a, k] += h
        elif which == "b":
            b[a] += h
        else:
            occ[a] += h
        return xyz, b, occ

    def same_pairs(self, which, a, k, h):
        base = self.pairs(self.xyz)[0]
        return all(np.array_equal(self.pairs(self.moved(which, a, k, s * h)[0])[0], base) for s in (-1.0, 1.0, -0.5, 0.5))


_scene = {}


def scene():
    if "s" not in _scene:
        _scene["s"] = Scene()
    return _scene["s"]


def parameters(sc):
    return [("xyz", a, k, H_XYZ) for a in range(len(sc.z)) for k in range(3)] + [("b", a, 0, H_B) for a in range(len(sc.z))] + [("occ", a, 0, H_OCC) for a in range(len(sc.z))]


def pick(grad, which, a, k):
    return float(grad["dXyz"][a, k] if which == "xyz" else (grad["dB"][a] if which == "b" else grad["dOcc"][a]))


def test_gradients_against_central_differences_of_the_weighted_sum():
    sc = scene()
    grad, got = sc.analytic(sc.w, sc.xyz, sc.b, sc.occ)
    assert got["nVoxels"].min() > 30
    compared = 0
    for which, a, k, h in parameters(sc):
        assert sc.same_pairs(which, a, k, h), (which, a, k)
        fd = {}
        for step in (h, 0.5 * h):
            (fp, mp), (fm, mm) = sc.weighted_sum(*sc.moved(which, a, k, step)), sc.weighted_sum(*sc.moved(which, a, k, -step))
            fd[step] = ((fp - fm) / (2.0 * step), (mp + mm) * 2.0 ** -50 / (2.0 * step))
        bound = abs(fd[h][0] - fd[0.5 * h][0]) + fd[0.5 * h][1]
        err = abs(pick(grad, which, a, k) - fd[0.5 * h][0])
        print("%s[%d][%d]: analytic %.12g, FD(h/2) %.12g, |difference| %.3g, bound %.3g" % (which, a, k, pick(grad, which, a, k), fd[0.5 * h][0], err, bound))
        assert err <= bound and abs(fd[0.5 * h][0]) > 100 * bound          # (the bound decides something: the derivative is resolved to 1 %)
        compared += 1
    assert compared == 5 * len(sc.z)


def test_gradients_of_the_profiled_target():
    """T(theta) = min over s, o of sum (obs - s calc - o)^2 / 2, s and o re-fitted at theta +- h; the analytic derivative is -s sum_v R d rho / d theta at
    the base point's s, o and residual R: the envelope argument.  obs is the model of displaced, re-weighted atoms plus noise."""
    sc = scene()
    rng = np.random.default_rng(77)
    truth = sc.density(sc.xyz + rng.normal(0.0, 0.15, size=sc.xyz.shape), sc.b * rng.uniform(0.8, 1.2, size=len(sc.b)), sc.occ)[0]
    obs = 0.7 * truth + 0.05 + rng.normal(0.0, 0.01, size=truth.shape)
    t0, s, o, res, _ = sc.target(obs, sc.xyz, sc.b, sc.occ)
    full = np.zeros((int(sc.header.ncrs[2]), int(sc.header.ncrs[1]), int(sc.header.ncrs[0])))
    full[sc.crs[:, 2], sc.crs[:, 1], sc.crs[:, 0]] = res
    grad, _ = sc.analytic(full, sc.xyz, sc.b, sc.occ)
    assert abs(s - 0.7) < 0.2 and t0 > 0
    for which, a, k, h in parameters(sc):
        assert sc.same_pairs(which, a, k, h)
        fd = {}
        for step in (h, 0.5 * h):
            tp, tm = sc.target(obs, *sc.moved(which, a, k, step)), sc.target(obs, *sc.moved(which, a, k, -step))
            fd[step] = ((tp[0] - tm[0]) / (2.0 * step), (tp[4] + tm[4]) * 2.0 ** -50 / (2.0 * step))
        bound = abs(fd[h][0] - fd[0.5 * h][0]) + fd[0.5 * h][1]
        analytic = -s * pick(grad, which, a, k)
        err = abs(analytic - fd[0.5 * h][0])
        print("T %s[%d][%d]: analytic %.12g, FD(h/2) %.12g, |difference| %.3g, bound %.3g" % (which, a, k, analytic, fd[0.5 * h][0], err, bound))
        assert err <= bound


def test_image_gradients_fold_through_a_two_fold():
    """Two copies of every atom, x and R x + t with R a 2-fold about z: the derivative of sum_v w (rho(x) + rho(R x + t)) with respect to x is the
    copy's gradient brought back through R^T, added to the atom's own; checked by central differences of the fp64 restatement."""
    from pdb_eda_amd import ccp4
    sc = scene()
    lo, hi = cases.box_of("box")
    centre = 0.5 * (lo + hi)
    rot = np.diag([-1.0, -1.0, 1.0])
    op = np.hstack([rot, (centre - rot.dot(centre))[:, None] + np.array([[0.3], [-0.2], [0.1]])])
    n = len(sc.z)
    rows = np.tile(np.arange(n), 2)

    def images(xyz):
        return np.concatenate([xyz, ccp4.applyOperator(op, xyz)])

    both = Scene()
    both.z, both.radii = np.tile(sc.z, 2), np.tile(sc.radii, 2)
    b2, occ2 = np.tile(sc.b, 2), np.tile(sc.occ, 2)
    grad, _ = both.analytic(both.w, images(sc.xyz), b2, occ2)
    folded = ccp4.foldImageGradients(grad, rows, np.array([np.eye(3)] * n + [rot] * n), n)
    assert np.array_equal(folded["dB"], grad["dB"][:n] + grad["dB"][n:]) and folded["dXyz"].shape == (n, 3)
    h = H_XYZ
    for a in range(n):
        for k in range(3):
            fd = {}
            for step in (h, 0.5 * h):
                plus, minus = sc.xyz.copy(), sc.xyz.copy()
                plus[a, k] += step
                minus[a, k] -= step
                assert np.array_equal(both.pairs(images(plus))[0], both.pairs(images(sc.xyz))[0]) and np.array_equal(both.pairs(images(minus))[0], both.pairs(images(sc.xyz))[0])
                (fp, mp), (fm, mm) = both.weighted_sum(images(plus), b2, occ2), both.weighted_sum(images(minus), b2, occ2)
                fd[step] = ((fp - fm) / (2.0 * step), (mp + mm) * 2.0 ** -50 / (2.0 * step))
            assert abs(folded["dXyz"][a, k] - fd[0.5 * h][0]) <= abs(fd[h][0] - fd[0.5 * h][0]) + fd[0.5 * h][1]
    # the fold is not the plain sum: the copy's x and y come back with the other sign
    assert not np.allclose(folded["dXyz"], grad["dXyz"][:n] + grad["dXyz"][n:])


def test_the_clamp_below_min_b_is_flat():
    from pdb_eda_amd import ccp4
    moments = np.array([[[1.0, 0.1, 0.2, 0.3, 2.0]]] * 3)
    grad = ccp4.gaussianAtomGradients(moments, [6, 6, 6], [2.0, 20.0, 7.0], [1.0, 1.0, 0.0], blur=3.0)
    assert grad["dB"][0] == 0.0 and grad["dB"][1] != 0.0 and grad["dB"][2] == 0.0          # (B + blur = 5 < 10; 23; 10 is not below: but occ = 0 has amp = 0)
    amp, expo, b = ccp4.gaussianAtomTerms([6], [20.0], [1.0], blur=3.0)
    assert grad["dB"][1] == amp[0] * (-1.5 * 1.0 / 23.0 + 4.0 * np.pi ** 2 * 2.0 / (23.0 * 23.0))
    assert np.array_equal(grad["dXyz"][1], (2.0 * expo[0] * amp[0]) * np.array([0.1, 0.2, 0.3]))
    assert grad["dOcc"][2] == 6 * (4 * np.pi / 10.0) ** 1.5 * 1.0 and grad["dOcc"][1] == amp[0]      # an occupancy of 0 has a derivative
    at_edge = ccp4.gaussianAtomGradients(moments[:1], [6], [7.0], [1.0], blur=3.0)
    assert at_edge["dB"][0] != 0.0                                                                  # B + blur == minB: the clamp is not active


def test_the_step_moves_a_displaced_gaussian_towards_the_truth():
    """One atom, obs = its own density: displaced by delta, the damped Gauss-Newton step points back (most of the way: the curvature is the
    isolated Gaussian's, the sum over voxels is close to its integral), T goes down, and the step never exceeds maxShift."""
    from pdb_eda_amd import ccp4
    sc = Scene(name="wide", n=1, seed=9)
    sc.radii = ccp4.modelRadii(ccp4.gaussianAtomTerms(sc.z, sc.b, sc.occ)[2], 4.0)
    lo, hi = cases.box_of("wide")
    sc.xyz = (0.5 * (lo + hi))[None, :] + np.array([[0.07, -0.04, 0.11]])
    obs = sc.density(sc.xyz, sc.b, sc.occ)[0]
    delta = np.array([[0.12, -0.08, 0.05]])
    moved = sc.xyz + delta
    t0, s, o, res, _ = sc.target(obs, moved, sc.b, sc.occ)
    full = np.zeros((int(sc.header.ncrs[2]), int(sc.header.ncrs[1]), int(sc.header.ncrs[0])))
    full[sc.crs[:, 2], sc.crs[:, 1], sc.crs[:, 0]] = res
    grad, _ = sc.analytic(full, moved, sc.b, sc.occ)
    grad_t = {k: -s * v for k, v in grad.items()}
    curv = ccp4.gaussianAtomCurvatures(sc.z, sc.b, sc.occ, sc.header.unitVolume)
    step = ccp4.gaussNewtonStep(grad_t, curv, s, ("xyz",), maxShift=0.3)
    assert np.all(step["b"] == 0) and np.all(step["occ"] == 0)
    along = float(step["xyz"][0].dot(-delta[0])) / float(delta[0].dot(delta[0]))
    t1 = sc.target(obs, moved + step["xyz"], sc.b, sc.occ)[0]
    print("step %s against delta %s: %.3f of the way back; T %.6g -> %.6g" % (step["xyz"][0], delta[0], along, t0, t1))
    assert along > 0 and t1 <= t0 and np.linalg.norm(moved + step["xyz"] - sc.xyz) < np.linalg.norm(delta)
    capped = ccp4.gaussNewtonStep(grad_t, curv, s, ("xyz",), maxShift=0.01)
    assert abs(np.linalg.norm(capped["xyz"][0]) - 0.01) < 1e-12 and np.allclose(np.cross(capped["xyz"][0], step["xyz"][0]), 0.0, atol=1e-12)
    assert sc.target(obs, moved + capped["xyz"], sc.b, sc.occ)[0] <= t0
