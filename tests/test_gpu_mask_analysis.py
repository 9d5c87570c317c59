"""The mask layer of DensityAnalysis on the MI355X path: molecule and solvent masks of the whole cell, their statistics, and the flat bulk-solvent
fit -- on a synthetic entry whose "observed" whole-cell map is MADE through the public API as model + k0 * inverse(scaled(fft(solventMask), B0))
with B0 on the fit's grid, so the fit has a known answer.

Bounds.  The maps are float32 (2^-24 relative per voxel) and the fit is linear least squares over thousands of coefficients, so rounding enters k
near 1e-7: k0 is asked for to 1e-4 relative, three decades above that.  For the same reason the FSC of the made map against model + solvent is
asked to be >= 0.9999 in every populated shell.  The solvent fraction is a count and is compared exactly with a numpy restatement of the mask
(spheres of radius + probe, then tests/spread_checker.py with the ball of the shrink radius under the below flag)."""
import io

import numpy as np
import pytest

import spread_checker as checker

pytestmark = pytest.mark.gpu

K0, B0 = 0.35, 50.0
EDGE, RESIDUES, SEED, SPACING = 64, 120, 7, 0.5          # (600 atoms and their mates in a 32 A cell: about a quarter of it is molecule)


def _analyzer(gpu_ctx, spec, st, rot, dens, diff, tag):
    from pdb_eda_amd import ccp4, densityAnalysis, structure, synthetic
    d = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, dens)), tag, ctx=gpu_ctx)
    f = ccp4.parse(io.BytesIO(synthetic.ccp4_bytes(spec, diff)), tag, ctx=gpu_ctx)
    densityAnalysis._attachCutoffs(d, f)
    return densityAnalysis.DensityAnalysis(tag, d, f, st, structure.PDBEntry(structure.PDBHeader(pdbid=tag, resolution=2.0, spaceGroup="P_1", rotationMats=rot)))


@pytest.fixture(scope="module")
def entry(gpu_ctx):
    """(the analyzer of the made map, the solvent mask's host copy): the first analyzer only lends its model and its mask."""
    from pdb_eda_amd import ccp4, densityAnalysis, synthetic
    spec, header, st, params, dens, diff, rot = synthetic.cube_entry((EDGE, EDGE, EDGE), RESIDUES, SEED)
    densityAnalysis.setGlobals(params)
    lender = _analyzer(gpu_ctx, spec, st, rot, dens, diff, "lender")
    observed, model = lender._fourierMaps()
    assert list(observed.header.ncrs) == [EDGE] * 3
    solvent = lender.solventMaskObj
    s2Max = ccp4.maxS2(observed.header)
    smooth = solvent.fourier().scale(ccp4.bFactorTable(B0, s2Max), s2Max).toMap()
    made = type(model._map).combine(model._map, smooth._map, K0)
    made = ccp4.DensityMatrix.fromDeviceMap(model.header, model.origin, made, "made", gpu_ctx).density
    return _analyzer(gpu_ctx, spec, st, rot, np.array(made), diff, "made"), np.array(solvent.density)


def test_bulk_solvent_fit_recovers_what_was_put_in(entry):
    analyzer, _ = entry
    fit = analyzer.bulkSolventFit()
    print("residuals per B:", fit["residuals"], "k_sol %.9g scale %.9g" % (fit["k_sol"], fit["scale"]))
    assert fit["b_sol"] == B0
    assert abs(fit["k_sol"] - K0) <= 1e-4 * K0
    assert abs(fit["scale"] - 1.0) <= 1e-4
    populated = fit["n"] > 0
    assert populated.sum() >= 15
    assert (fit["fsc_after"][populated] >= 0.9999).all() and (fit["fsc_before"][populated] <= fit["fsc_after"][populated] + 1e-12).all()
    assert (fit["fsc_before"][populated] < 0.9999).any()          # (without the solvent the low shells are off: the reason for the model)


def test_solvent_shell_table(entry):
    analyzer, _ = entry
    table = analyzer.solventShellTable()
    populated = table["n"] > 0
    print("fsc with solvent:", np.array2string(table["fsc"], precision=7))
    assert (table["fsc"][populated] >= 0.9999).all()
    plain = analyzer.modelShellTable()
    assert float(plain["fsc"][populated].min()) < 0.9999
    masked = analyzer.maskedModelShellTable()
    assert np.array_equal(masked["n"], plain["n"]) and np.isfinite(masked["fsc"][populated]).all()


def _solvent_restatement(analyzer, shape):
    """The solvent mask in numpy: the grown spheres voxel by voxel (float64 distances against float32 radii, each sphere inside its own box of
    voxels), then the checker's spread of the uncovered voxels by the ball of the shrink radius.  Also the least distance of a voxel from a sphere."""
    from pdb_eda_amd import ccp4, densityAnalysis
    header = analyzer._fourierMaps()[0].header
    xyz, radii = analyzer._maskAtoms(header, densityAnalysis.maskProbe)
    grown_r = (np.asarray(radii, dtype=np.float64) + densityAnalysis.maskProbe).astype(np.float32).astype(np.float64)
    ns, nr, nc = shape
    covered = np.zeros(shape, dtype=bool)
    origin = np.array(header.crs2xyzCoord([0, 0, 0]), dtype=np.float64)
    assert header.orthogonal and np.allclose(header.crs2xyzCoord([1, 2, 3]), origin + SPACING * np.array([1, 2, 3]))      # x, y, z run along c, r, s
    margin = np.inf
    for a in range(len(xyz)):
        lo = np.floor((xyz[a] - origin - grown_r[a]) / SPACING).astype(int) - 1
        hi = np.ceil((xyz[a] - origin + grown_r[a]) / SPACING).astype(int) + 1
        lo, hi = np.maximum(lo, 0), np.minimum(hi, [nc - 1, nr - 1, ns - 1])
        if (lo > hi).any():
            continue
        c, r, s = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[2], hi[2] + 1), indexing="ij")
        pos = header.crs2xyz_array(np.stack([c, r, s], axis=-1).reshape(-1, 3).astype(np.float64))
        d = np.sqrt(((pos - xyz[a]) ** 2).sum(axis=1))
        margin = min(margin, float(np.abs(d - grown_r[a]).min()))
        inside = (d <= grown_r[a]).reshape(c.shape)
        covered[s[inside], r[inside], c[inside]] = True
    ball = ccp4.spreadTable(header, densityAnalysis.maskShrink)[0]
    values = np.append(np.ones(len(ball), dtype=np.float32), np.float32(0.0))
    return checker.spread(covered.astype(np.float32), ball, values, [int(v) for v in header.crsInterval], 0.5, below=True), margin


def test_mask_summary_counts_the_solvent_exactly(entry):
    analyzer, solvent = entry
    want, margin = _solvent_restatement(analyzer, solvent.shape)
    assert margin > 1e-6          # (no voxel's membership hinges on an ulp)
    assert np.array_equal(solvent.view(np.uint32), want.view(np.uint32))
    summary = analyzer.maskSummary()
    n = int((want > 0.5).sum())
    assert 0.2 < n / want.size < 0.9
    assert summary["solvent_voxels"] == n and summary["cell_voxels"] == want.size and summary["solvent_fraction"] == n / want.size
    diff = np.asarray(analyzer._wholeCellDiff().density, dtype=np.float64)
    inside = want > 0.5
    assert abs(summary["solvent_noise"] - float(diff[inside].std())) <= 1e-9 and abs(summary["protein_diff_mean"] - float(diff[~inside].mean())) <= 1e-9
    dens = np.asarray(analyzer._fourierMaps()[0].density, dtype=np.float64)
    assert abs(summary["solvent_density_mean"] - float(dens[inside].mean())) <= 1e-9 and abs(summary["protein_density_std"] - float(dens[~inside].std())) <= 1e-9
    molecule = np.asarray(analyzer.moleculeMaskObj.density)
    assert set(np.unique(molecule)) == {0.0, 1.0} and not (molecule.astype(bool) & inside).any()          # (the molecule lies inside the grown spheres)


def test_mask_mode_prints_both_levels(entry):
    from pdb_eda_amd import singleStructure
    analyzer, _ = entry
    header, rows = singleStructure.rows(analyzer, "mask", "summary")
    assert len(rows) == 1 and len(rows[0]) == len(header) and rows[0][header.index("b_sol")] == B0
    assert abs(rows[0][header.index("k_sol")] - K0) <= 1e-4 * K0
    text = singleStructure.dumps(header, rows)
    assert '"solvent_fraction"' in text and '"solvent_noise"' in text
    header, rows = singleStructure.rows(analyzer, "mask", "shell")
    assert header == analyzer.maskShellHeader and len(rows) == 20 and all(len(row) == len(header) for row in rows)
    assert "fsc_with_solvent" in singleStructure.dumps(header, rows, "csv").splitlines()[0]
    with pytest.raises(ValueError):
        singleStructure.rows(analyzer, "mask", "atom")
