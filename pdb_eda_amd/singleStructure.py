"""Single-structure result tables and writers (ref pdb_eda/singleStructure.py:57-196).

The reference's ``pdb_eda single`` is a docopt CLI around one ``DensityAnalysis`` object; the CLI
is out of scope here (docopt / jsonpickle are not available), the *results* are not: ``TABLES`` maps every sub-mode to the header
and the ``DensityAnalysis`` call the reference's ``main`` uses for it (singleStructure.py:98-163), ``rows`` looks the
sub-mode up, and ``write`` emits the reference's JSON / CSV text (169-178), so
outputs diff cleanly against reference runs made elsewhere.  All numbers come from the MI355X path
behind ``DensityAnalysis``.
"""
import json
import sys

import numpy

from . import densityAnalysis

MODES = ("cloud", "density", "difference", "blob", "statistics", "peak", "profile", "partition", "shape", "dipole", "basin", "qscore", "model", "local", "fourier", "mask", "refine", "fit")


def numpyConverter(obj):
    """Values json.dumps cannot write (numpy scalars / arrays) as plain Python ones (role of singleStructure.py:180-196)."""
    if isinstance(obj, numpy.generic):
        return obj.item()
    if isinstance(obj, numpy.ndarray):
        return [numpyConverter(item) for item in obj]
    return obj


def _plainColumns(table, listColumns=(), floatColumns=()):
    """Tuples / arrays in the given columns become lists (of floats) so every row serialises (singleStructure.py:119-121 ...)."""
    for row in table:
        for c in listColumns:
            row[c] = list(row[c])
        for c in floatColumns:
            row[c] = [float(v) for v in row[c]]
    return table


def _blobTable(analyzer, o):
    """blob sub-mode: statistics of the green and / or red Fo-Fc blobs, else of the blue 2Fo-Fc blobs (singleStructure.py:128-141)."""
    diffObj, densObj, numSD = analyzer.diffDensityObj, analyzer.densityObj, o["numSD"]
    if o["green"] and o["red"]:          # one fused pass over the Fo-Fc grid gives both lists
        lists = diffObj.createFullBlobLists(diffObj.meanDensity + numSD * diffObj.stdDensity)
    elif o["green"]:
        lists = [diffObj.createFullBlobList(diffObj.meanDensity + numSD * diffObj.stdDensity)]
    elif o["red"]:
        lists = [diffObj.createFullBlobList(-1 * (diffObj.meanDensity + numSD * diffObj.stdDensity))]
    else:
        lists = [densObj.createFullBlobList(densObj.meanDensity + numSD * densObj.stdDensity)]
    table = [row for blobs in lists for row in analyzer.calculateAtomSpecificBlobStatistics(blobs)]
    return _plainColumns(table, listColumns=(9,), floatColumns=(10, 11))


def _peakLists(analyzer, o):
    """The peak lists of the peak and basin sub-modes: green and / or red Fo-Fc, else blue 2Fo-Fc, with the blob lists at the same cutoff."""
    diffObj, densObj, numSD = analyzer.diffDensityObj, analyzer.densityObj, o["numSD"]
    if o["green"] and o["red"]:          # one fused pass over the Fo-Fc grid gives both lists
        cut = diffObj.meanDensity + numSD * diffObj.stdDensity
        lists = diffObj.findPeakLists(cut, diffObj.createFullBlobLists(cut))
    elif o["green"] or o["red"]:
        cut = (1 if o["green"] else -1) * (diffObj.meanDensity + numSD * diffObj.stdDensity)
        lists = [diffObj.findPeaks(cut, diffObj.createFullBlobList(cut))]
    else:
        cut = densObj.meanDensity + numSD * densObj.stdDensity
        lists = [densObj.findPeaks(cut, densObj.createFullBlobList(cut))]
    return lists


def _peakTable(analyzer, o):
    """peak sub-mode (no reference counterpart): the local extrema of the green and / or red Fo-Fc map, else of the blue 2Fo-Fc
    map, each with its blob of the blob sub-mode's list at the same cutoff and its nearest symmetry atom."""
    table = [row for peaks in _peakLists(analyzer, o) for row in analyzer.calculateAtomSpecificPeakStatistics(peaks)]
    return _plainColumns(table, listColumns=(10,), floatColumns=(11, 12))


def _basinTable(analyzer, o):
    """basin sub-mode (no reference counterpart): the peak sub-mode's rows, each with the voxels, electrons and share of its blob that belong to
    the peak, the pass to the adjacent peak and the prominence."""
    table = [row for peaks in _peakLists(analyzer, o) for row in analyzer.calculateAtomSpecificBasinStatistics(peaks)]
    return _plainColumns(table, listColumns=(10,), floatColumns=(11, 12, 20))


def _shapeTable(analyzer, o):
    """shape sub-mode (no reference counterpart): extent, elongation and strongest voxel of the blobs of the blob sub-mode's lists -- the green and / or
    red Fo-Fc blobs, else the blue 2Fo-Fc blobs -- each with the symmetry atom nearest to its strongest voxel."""
    diffObj, densObj, numSD = analyzer.diffDensityObj, analyzer.densityObj, o["numSD"]
    if o["green"] and o["red"]:          # one fused pass over the Fo-Fc grid gives both lists
        lists = diffObj.createFullBlobLists(diffObj.meanDensity + numSD * diffObj.stdDensity)
    elif o["green"] or o["red"]:
        lists = [diffObj.createFullBlobList((1 if o["green"] else -1) * (diffObj.meanDensity + numSD * diffObj.stdDensity))]
    else:
        lists = [densObj.createFullBlobList(densObj.meanDensity + numSD * densObj.stdDensity)]
    table = [row for blobs in lists for row in analyzer.calculateBlobShapeStatistics(blobs)]
    return _plainColumns(table, listColumns=(19,), floatColumns=(7, 12, 20))


def _dipoleTable(analyzer, o):
    """dipole sub-mode (no reference counterpart): the green Fo-Fc blobs that have a red one beside them -- the fused lists of the blob sub-mode at
    ``numSD`` -- each with its red partner, the gap, the shift vector and the symmetry atom between them; ``radius`` is the largest gap when given."""
    diffObj, numSD = analyzer.diffDensityObj, o["numSD"]
    green, red = diffObj.createFullBlobLists(diffObj.meanDensity + numSD * diffObj.stdDensity)
    table = analyzer.calculateBlobDipoles(green, red, o["radius"]) if o["radiusGiven"] else analyzer.calculateBlobDipoles(green, red)
    return _plainColumns(table, listColumns=(15,), floatColumns=(8, 9, 16))


def _partitionBlobTable(analyzer, o):
    """partition / blob: who owns the voxels of the green and / or red Fo-Fc blobs (green when neither is asked for)."""
    diffObj, numSD = analyzer.diffDensityObj, o["numSD"]
    cut = diffObj.meanDensity + numSD * diffObj.stdDensity
    if o["green"] and o["red"]:
        lists = diffObj.createFullBlobLists(cut)
    else:
        lists = [diffObj.createFullBlobList(-cut if o["red"] else cut)]
    table = [row for blobs in lists for row in analyzer.calculateBlobOwnership(blobs, o["radius"])]
    for row in table:      # (the owner's symmetry tag as a list, like the blob table's; None where nobody owns a voxel of the blob)
        row[7] = None if row[7] is None else list(row[7])
    return table


def _partitionSummaryTable(analyzer, o):
    summary = analyzer.partitionSummary(o["radius"], o["numSD"])
    return [[summary[name] for name in _PARTITION_SUMMARY]]


def _qScoreSummaryTable(analyzer, o):
    summary = analyzer.qScoreSummary()
    return [[summary[name] for name in _QSCORE_SUMMARY]]


def _modelSummaryTable(analyzer, o):
    summary = analyzer.modelSummary()
    return [[summary[name] for name in _MODEL_SUMMARY]]


def _refineSummaryTable(analyzer, o):
    summary = analyzer.refineSummary()
    return [[summary[name] for name in _REFINE_SUMMARY]]


def _localSummaryTable(analyzer, o):
    summary = analyzer.localSummary()
    return [[summary[name] for name in _LOCAL_SUMMARY]]


def _fourierSummaryTable(analyzer, o):
    summary = analyzer.fourierSummary(o["shells"])
    return [[summary[name] for name in _FOURIER_SUMMARY]]


def _maskSummaryTable(analyzer, o):
    summary = dict(analyzer.maskSummary())
    fit = analyzer.bulkSolventFit(nShells=o["shells"])
    summary.update({"k_sol": fit["k_sol"], "b_sol": fit["b_sol"], "solvent_scale": fit["scale"], "solvent_residual": fit["residual"]})
    return [[summary[name] for name in _MASK_SUMMARY]]


_MASK_SUMMARY = ["cell_voxels", "solvent_voxels", "solvent_fraction"] + ["%s_%s_%s" % (region, name, what) for region in ("solvent", "protein") for name in ("density", "diff")
                                                                       for what in ("mean", "std")] + ["solvent_noise", "k_sol", "b_sol", "solvent_scale", "solvent_residual"]
_REFINE_SUMMARY = ["num_atoms", "cycles", "target_before", "target_after", "cc_before", "cc_after", "scale_before", "scale_after", "rms_shift", "rms_delta_b"]
_FOURIER_SUMMARY = ["grid_c", "grid_r", "grid_s", "d_min", "num_shells", "fsc_05_resolution", "fsc_0143_resolution", "overall_fsc", "overall_scale"]
_LOCAL_SUMMARY = ["window_sigma", "window_truncate", "radius_c", "radius_r", "radius_s", "num_local_green_blobs", "num_local_red_blobs", "num_green_blobs", "num_red_blobs",
                  "median_atom_local_cc", "min_atom_local_cc"]
_MODEL_SUMMARY = ["cc", "scale", "offset", "n", "electrons_placed", "electrons_found"]
_QSCORE_SUMMARY = [cls + "_" + what for cls in ("all", "backbone", "side_chain", "water") for what in ("mean_q_score", "median_q_score", "num_atoms")]
_PARTITION_SUMMARY = ["max_distance", "num_sd", "box_voxels", "asymmetric_unit_voxels", "symmetry_voxels", "unowned_voxels", "unowned_fraction", "unowned_mean",
                      "unowned_std", "map_mean", "map_std"] + [prefix + cls + "_" + sign + "_discrepancy" for cls in ("asymmetric_unit", "symmetry", "unowned")
                                                              for sign in ("positive", "negative") for prefix in ("", "num_electrons_")]


def _cloudTable(attribute):
    def table(analyzer, o):
        return [[numpyConverter(v) for v in item] + [analyzer.densityElectronRatio] for item in getattr(analyzer, attribute)]
    return table


_DA = densityAnalysis.DensityAnalysis
# Columns main() turns into lists for JSON: 4 and 5 = symmetry tag and coordinate of the atom-metrics rows.  The reference
# applies the SAME indices to the symmetry-atom density / discrepancy rows (singleStructure.py:119-121, 133-135), whose
# leading 'model' column shifts them onto atom_name (-> list of characters) and symmetry (-> floats): reproduced as is (Q11).
_SYM = dict(listColumns=(4,), floatColumns=(5,))
# (mode, level) -> (header of the table, rows of the table): one entry per sub-mode of `pdb_eda single` (singleStructure.py:97-163)
TABLES = {
    ("cloud", "atom"): (lambda an: list(map(str, an.atomCloudDescriptions.dtype.names)) + ['density_electron_ratio'], _cloudTable("atomCloudDescriptions")),
    ("cloud", "residue"): (lambda an: _DA.residueCloudHeader + ['density_electron_ratio'], _cloudTable("residueCloudDescriptions")),
    ("cloud", "domain"): (lambda an: _DA.domainCloudHeader + ['density_electron_ratio'], _cloudTable("domainCloudDescriptions")),
    ("density", "atom"): (lambda an: _DA.atomRegionDensityHeader,
                          lambda an, o: an.calculateAtomRegionDensity(o["radius"], o["numSD"], o["type"], o["optimizedRadii"])),
    ("density", "residue"): (lambda an: _DA.residueRegionDensityHeader,
                             lambda an, o: an.calculateResidueRegionDensity(o["radius"], o["numSD"], o["type"], o["atomMask"], o["optimizedRadii"])),
    ("density", "symmetry-atom"): (lambda an: _DA.symmetryAtomRegionDensityHeader,
                                   lambda an, o: _plainColumns(an.calculateSymmetryAtomRegionDensity(o["radius"], o["numSD"], o["type"], o["optimizedRadii"]), **_SYM)),
    ("difference", "atom"): (lambda an: _DA.atomRegionDiscrepancyHeader, lambda an, o: an.calculateAtomRegionDiscrepancies(o["radius"], o["numSD"], o["type"])),
    ("difference", "residue"): (lambda an: _DA.residueRegionDiscrepancyHeader,
                                lambda an, o: an.calculateResidueRegionDiscrepancies(o["radius"], o["numSD"], o["type"], o["atomMask"])),
    ("difference", "symmetry-atom"): (lambda an: _DA.symmetryAtomRegionDiscrepancyHeader,
                                      lambda an, o: _plainColumns(an.calculateSymmetryAtomRegionDiscrepancies(o["radius"], o["numSD"], o["type"]), **_SYM)),
    ("blob", None): (lambda an: _DA.blobStatisticsHeader, _blobTable),
    ("peak", None): (lambda an: _DA.peakStatisticsHeader, _peakTable),
    ("basin", None): (lambda an: _DA.basinStatisticsHeader, _basinTable),
    ("shape", None): (lambda an: _DA.blobShapeHeader, _shapeTable),
    ("dipole", None): (lambda an: _DA.blobDipoleHeader, _dipoleTable),
    # (no reference counterpart; the shell columns are lists, carried as the peak table's list columns are)
    ("profile", "atom"): (lambda an: _DA.atomRadialProfileHeader, lambda an, o: an.calculateAtomRadialProfiles(o["radius"], o["shells"], o["numSD"], o["type"])),
    ("profile", "atom-type"): (lambda an: _DA.atomTypeRadialProfileHeader, lambda an, o: an.atomTypeRadialProfiles(o["radius"], o["shells"], o["numSD"])),
    # (no reference counterpart: the Fo-Fc map partitioned among the symmetry atoms; ``radius`` is the maximum distance)
    ("partition", "atom"): (lambda an: _DA.atomPartitionHeader, lambda an, o: an.calculateAtomPartitionDiscrepancies(o["radius"], o["numSD"], o["type"])),
    ("partition", "residue"): (lambda an: _DA.residuePartitionHeader, lambda an, o: an.calculateResiduePartitionDiscrepancies(o["radius"], o["numSD"], o["type"])),
    ("partition", "summary"): (lambda an: list(_PARTITION_SUMMARY), _partitionSummaryTable),
    ("partition", "blob"): (lambda an: _DA.blobOwnershipHeader, _partitionBlobTable),
    # (no reference counterpart: Q-scores over the 2Fo-Fc map, all symmetry atoms competing for the sample points)
    ("qscore", "atom"): (lambda an: _DA.atomQScoreHeader, lambda an, o: an.calculateAtomQScores(o["type"])),
    ("qscore", "residue"): (lambda an: _DA.residueQScoreHeader, lambda an, o: an.calculateResidueQScores(o["type"])),
    ("qscore", "summary"): (lambda an: list(_QSCORE_SUMMARY), _qScoreSummaryTable),
    # (no reference counterpart: the 2Fo-Fc map against the density calculated from the symmetry atoms; ``radius`` is the sphere's when given, else atomMetrics')
    ("model", "atom"): (lambda an: _DA.atomModelCorrelationHeader, lambda an, o: an.calculateAtomModelCorrelations(o["radius"] if o["radiusGiven"] else None)),
    ("model", "residue"): (lambda an: _DA.residueModelCorrelationHeader, lambda an, o: an.calculateResidueModelCorrelations(o["radius"] if o["radiusGiven"] else None)),
    ("model", "summary"): (lambda an: list(_MODEL_SUMMARY), _modelSummaryTable),
    # (no reference counterpart: the Fo-Fc map against its LOCAL noise level, the 2Fo-Fc map against the model inside a window; no option applies)
    ("local", "atom"): (lambda an: _DA.atomLocalHeader, lambda an, o: an.calculateAtomLocalCorrelations()),
    ("local", "residue"): (lambda an: _DA.residueLocalHeader, lambda an, o: an.calculateResidueLocalCorrelations()),
    ("local", "summary"): (lambda an: list(_LOCAL_SUMMARY), _localSummaryTable),
    # (no reference counterpart: the whole-cell 2Fo-Fc map against the model in reciprocal space; ``shells`` is the number of resolution shells)
    ("fourier", "shell"): (lambda an: _DA.fourierShellHeader, lambda an, o: an.calculateFourierShells(o["shells"])),
    ("fourier", "summary"): (lambda an: list(_FOURIER_SUMMARY), _fourierSummaryTable),
    # (no reference counterpart: the whole cell divided into molecule and solvent, the flat bulk-solvent fit; ``shells`` is the number of resolution shells)
    ("mask", "shell"): (lambda an: _DA.maskShellHeader, lambda an, o: an.calculateMaskShells(o["shells"])),
    ("mask", "summary"): (lambda an: list(_MASK_SUMMARY), _maskSummaryTable),
    # (no reference counterpart: real-space refinement of the deposited atoms against the 2Fo-Fc map, x, y, z and B; no option applies)
    ("refine", "atom"): (lambda an: _DA.refineAtomHeader, lambda an, o: an.refineAtoms()),
    ("refine", "summary"): (lambda an: list(_REFINE_SUMMARY), _refineSummaryTable),
    # (no reference counterpart: a rigid fragment -- a residue of the structure, named by ``type`` -- tried in every green blob that can hold it; blob: the best pose per blob)
    ("fit", "blob"): (lambda an: _DA.blobFitHeader, lambda an, o: an.calculateBlobFits(an.defaultFitFragment(o["type"]))),
    ("statistics", "residue"): (lambda an: an.residueMetricsHeaderList, lambda an, o: an.residueMetrics()),
    ("statistics", "atom"): (lambda an: an.atomMetricsHeaderList, lambda an, o: _plainColumns(an.atomMetrics(), **_SYM)),
}


def rows(analyzer, mode, level="atom", radius=None, numSD=None, type="", atomMask=None, optimizedRadii=False, green=False, red=False,
         includePdbid=False, shells=20):
    """(headerList, rowList) of one ``pdb_eda single`` sub-mode, looked up in ``TABLES``.

    mode: cloud | density | difference | blob | statistics | peak | profile | partition | shape | dipole | basin | qscore | model | local | fourier | mask | refine | fit;  level: atom | residue | domain | symmetry-atom
    (the reference's --atom / --residue / --domain / --symmetry-atom; ignored by blob, peak, basin, shape and dipole) | atom-type (profile) | summary | blob
    (partition) | summary (qscore: atom | residue | summary, no other option applies; model: atom | residue | summary, ``radius`` is the sphere's, by default the one of the statistics mode; local: atom | residue | summary under the module's window, no other option applies; fourier: shell | summary, ``shells`` resolution shells; mask: shell | summary, ``shells`` resolution shells; refine: atom | summary, no option applies; fit: blob, ``type`` names the residue whose atoms are the fragment);  green / red: blob / peak / basin / shape colours (neither = blue);  numSD default 3.0 for green / red / difference / partition, else 1.5
    (singleStructure.py:65-67);  profile: ``radius`` is the profile's maxRadius, cut into ``shells`` shells;  partition: ``radius`` is the
    maximum distance of a voxel from its owner, green / red pick the blob level's lists (green alone by default);  dipole: always the fused green
    and red lists (numSD default 3.0), ``radius`` is the largest gap between the two blobs when given (else 2.5 A);  radius default 3.5 elsewhere."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % (MODES,))
    key = (mode, None if mode in ("blob", "peak", "shape", "dipole", "basin") else level)
    if key not in TABLES:
        raise ValueError("%s mode has the levels %s" % (mode, ", ".join(lv for md, lv in TABLES if md == mode and lv)))
    options = {"radius": float(radius if radius is not None else 3.5), "radiusGiven": radius is not None,
               "numSD": float(numSD if numSD is not None else (3.0 if green or red or mode in ("difference", "partition", "dipole") else 1.5)),
               "type": type, "atomMask": atomMask, "optimizedRadii": optimizedRadii, "green": green, "red": red, "shells": int(shells)}
    if mode == "cloud":
        analyzer.aggregateCloud()
    header, table = TABLES[key]
    headerList, result = list(header(analyzer)), table(analyzer, options)
    if includePdbid:
        headerList = ["pdbid"] + headerList
        result = [[analyzer.pdbid] + list(row) for row in result]
    return headerList, result


def validationLine(analyzer):
    """The text ``pdb_eda single ... statistics --print-validation`` prints (singleStructure.py:146-148)."""
    medianAbsFo, medianAbsFc = analyzer.medianAbsFoFc()
    return "Median abs Fo(<1sd): %s Median abs Fc(<1sd): %s Relative Difference: %s" % (medianAbsFo, medianAbsFc, (medianAbsFo - medianAbsFc) / max(medianAbsFo, medianAbsFc))


def dumps(headerList, result, outFormat="json"):
    """The text the reference writes (singleStructure.py:169-178): CSV = header row + str() of every cell joined by
    commas; JSON = list of {header: value} objects, indent 2, sorted keys."""
    if outFormat == 'csv':
        return '\n'.join(','.join(map(str, row)) for row in [headerList] + list(result)) + '\n'
    return json.dumps([dict(zip(headerList, [numpyConverter(v) for v in row])) for row in result], indent=2, sort_keys=True) + '\n'


def write(headerList, result, outFile="-", outFormat="json"):
    text = dumps(headerList, result, outFormat)
    if outFile == "-":
        sys.stdout.write(text)
    else:
        with open(outFile, 'w') as fh:
            fh.write(text)
