"""Optimise mode: the radius descent of ``pdb_eda optimize`` over GPU-resident entries.

``optimize`` restates the reference's ``optimizeParams.main`` (optimizeParams.py:115-327): one first evaluation, the choice of
the starting atom type, then the ``while True`` loop with its accept / reject rule, its step-size rules and its stop rules.
An evaluation is ``evaluator.iteration(params)`` -- ``optimizeSweep.Sweep`` / ``ProcessSweep`` re-analyse the entries they
keep resident in HBM and reduce the records over every rank (``optimizeStats``).  The descent itself is a few dozen scalar
decisions per iteration on the host.

The decision rules are the reference's to the bit, quirks included (each one is marked where it happens), so a run here picks
the same steps and writes the same parameter file as a reference run given the same medians.  Every rank runs the same
decisions on the same all-gathered reduction; only rank 0 writes files.

Deliberate differences from the reference:
  * an unreadable params file or an unknown ``startAtomType`` raises ``ValueError`` (the reference builds a ``RuntimeError``
    and never raises it);
  * no ``.execution_times`` file: entries stay resident where they were loaded and are sharded once, by ``cost_hint``;
  * no docopt command line, like every other mode of this package: ``optimize`` / ``run`` / ``compare`` / ``finalize`` are
    the interface.
"""
import datetime
import json
import os
import random
import sys

import numpy as np

from . import densityAnalysis, multipleStructures, optimizeStats, optimizeSweep


def dumpParams(params):
    """The text of a params file as the reference writes it (``print(json.dumps(..., indent=2, sort_keys=True))``)."""
    return json.dumps(params, indent=2, sort_keys=True) + "\n"


def writeParams(path, params):
    with open(path, "w") as fh:
        fh.write(dumpParams(params))


def loadParams(source):
    """A params table from a dict (copied) or the path of a JSON file; ``ValueError`` if it cannot be read or parsed."""
    if isinstance(source, dict):
        return dict(source)
    try:
        with open(source, "r") as fh:
            params = json.load(fh)
    except (OSError, ValueError, TypeError) as exception:
        raise ValueError('params file "%s" does not exist or is not parsable (%s)' % (source, exception))
    if not isinstance(params, dict):
        raise ValueError('params file "%s" does not hold a parameter table' % source)
    return params


def _rank_world():
    try:
        import torch.distributed as dist
    except ImportError:
        return 0, 1
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


class _Log(object):
    """The log file of rank 0 (a path or an open text file); every other rank, or ``log=None``, writes nothing."""

    def __init__(self, log, enabled):
        self._fh, self._own = None, False
        if enabled and log is not None:
            if hasattr(log, "write"):
                self._fh = log
            else:
                self._fh, self._own = open(log, "w"), True

    def __call__(self, *values):
        if self._fh is not None:
            print(*values, file=self._fh)

    def close(self):
        if self._own:
            self._fh.close()
        elif self._fh is not None:
            self._fh.flush()


def _summary(log, medianDiffs, meanDiffs, overallStdDevDiffs, penalties, sizes, maxSize, maxOverlapCompleteness, atomTypes2Optimize):
    """ref optimizeParams.py:231-246 (and 171-186): the per-evaluation summary lines of the log."""
    selected = [t for t in medianDiffs.keys() if not atomTypes2Optimize or t in atomTypes2Optimize]
    log("Max Absolute Weighted Median Diff:", max([abs(medianDiffs[t] * sizes[t] / maxSize) for t in selected]),
        ", Weighted Diff StdDev:", overallStdDevDiffs, ", Max Size:", maxSize)
    log("Max Absolute Median Diff:", max([abs(medianDiffs[t]) for t in selected]),
        ", Max Abs Diff Mean-Median:", max([abs(meanDiffs[t] - medianDiffs[t]) for t in selected]),
        ", Mean Abs Diff Mean-Median:", np.mean([abs(meanDiffs[t] - medianDiffs[t]) for t in selected]))
    log("Max Absolute Weighted Penalty:", max([abs(penalties[t] * sizes[t] / maxSize) for t in penalties.keys() if not atomTypes2Optimize or t in atomTypes2Optimize]),
        ", max overlap completeness=", maxOverlapCompleteness)


def optimize(params, evaluator, *, maxIncrement=0.2, minIncrement=0.001, startRadius=0.0, startAtomType="", stop=0.0,
             unweighted=False, inversePenaltyWeight=3.0, ignore=False, reverse=False, log=None, outParamsPath=None,
             maxIterations=None):
    """ref optimizeParams.py:115-327: the steepest-descent search over the atom-type radii.

    ``params``: the start table (a dict, or the path of a params file).  ``evaluator.iteration(table)`` returns
    ``((medianDiffs, meanDiffs, overallStdDevDiffs, medianSlopes, sizes, overlapCompleteness), records)`` -- what ``Sweep`` /
    ``ProcessSweep`` return.  The keywords are the reference's options (``--max``, ``--min``, ``--radius``, ``--start``,
    ``--stop``, ``--unweighted``, ``--penalty-weight``, ``--ignore``, ``--reverse``); ``log`` is a path or an open text file;
    ``outParamsPath`` receives ``.temp`` after every accepted step and the result at the end.  ``maxIterations`` caps the
    loop (None: run until a stop rule ends it, as the reference does).

    Returns ``(outParams, trace)``: ``trace`` holds one dict per evaluation of the loop -- atom type, previous and tested
    radius, increment, penalty, the best penalty it was compared with, accepted or not, and the evaluation's medians and
    penalties."""
    params = loadParams(params)
    if "radii" not in params or "slopes" not in params:
        raise ValueError("params table without 'radii' / 'slopes'")
    if maxIterations is not None and int(maxIterations) < 1:
        raise ValueError("maxIterations must be at least 1 (or None)")
    maxRadiusIncrement = float(maxIncrement)
    radiusIncrement = maxRadiusIncrement
    minRadiusIncrement = float(minIncrement)
    stoppingFractionalDifference = float(stop)
    startingRadius = float(startRadius)
    inversePenaltyWeight = float(inversePenaltyWeight)
    if not (minRadiusIncrement > 0 and maxRadiusIncrement >= minRadiusIncrement):
        raise ValueError("need 0 < minIncrement <= maxIncrement")

    currentRadii = dict(params["radii"])
    atomTypes2Optimize = None
    if not ignore and "optimize" in params:
        atomTypes2Optimize = set(params["optimize"])
    if reverse and atomTypes2Optimize:
        atomTypes2Optimize = {t for t in currentRadii.keys() if t not in atomTypes2Optimize}
    if startAtomType != "" and startAtomType not in currentRadii:
        raise ValueError('starting atom "%s" is not valid' % startAtomType)

    rank, _ = _rank_world()
    log = _Log(log, rank == 0)
    try:
        log("Options:", {"maxIncrement": maxRadiusIncrement, "minIncrement": minRadiusIncrement, "startRadius": startingRadius,
                         "startAtomType": startAtomType, "stop": stoppingFractionalDifference, "unweighted": bool(unweighted),
                         "inversePenaltyWeight": inversePenaltyWeight, "ignore": bool(ignore), "reverse": bool(reverse),
                         "maxIterations": maxIterations})
        log("Calculating start median differences: start-time=", str(datetime.datetime.now()))

        (bestMedianDiffs, meanDiffs, overallStdDevDiffs, medianSlopes, sizes, overlapCompleteness), _ = \
            evaluator.iteration({**params, "radii": dict(currentRadii), "slopes": dict(params["slopes"])})
        # Quirk (ref 165): slopes start as the medians with the table's own slopes on top, so the table's slopes win; and since every
        # accepted step merges {**slopes, **currentSlopes} (ref 260), the current value keeps winning: slopes are effectively frozen.
        currentSlopes = {**medianSlopes, **(params["slopes"])}
        maxOverlapCompleteness = max(overlapCompleteness.values())
        bestPenalties = optimizeSweep.penalties(bestMedianDiffs, overlapCompleteness, inversePenaltyWeight)

        maxSize = max([sizes[t] for t in bestMedianDiffs.keys() if not atomTypes2Optimize or t in atomTypes2Optimize])
        log("Starting Radii Min-Max: [", min(currentRadii.values()), ",", max(currentRadii.values()), "]")
        _summary(log, bestMedianDiffs, meanDiffs, overallStdDevDiffs, bestPenalties, sizes, maxSize, maxOverlapCompleteness, atomTypes2Optimize)
        log("Overlap Completeness Min-Max: [", min(overlapCompleteness.values()), ",", max(overlapCompleteness.values()), "]")
        log("Radii:", currentRadii)
        log("Median Diffs:", bestMedianDiffs)
        log("Overlap Completeness:", overlapCompleteness)
        log("Penalties:", bestPenalties)

        # ref 195-207.  Ties in max() go to the first key in params["radii"] order (dicts keep it all the way through optimizeStats).
        testBestPenalties = {t: p for (t, p) in bestPenalties.items() if t in atomTypes2Optimize} if atomTypes2Optimize else bestPenalties
        if unweighted:
            currentAtomType = max(testBestPenalties, key=lambda y: abs(testBestPenalties[y])) if not startAtomType else startAtomType
        else:
            # Quirk: abs(p * size) here, abs(p) * size in the loop (ref 199 vs 286).
            currentAtomType = max(testBestPenalties, key=lambda y: abs(testBestPenalties[y] * sizes[y])) if not startAtomType else startAtomType
        previousRadius = currentRadii[currentAtomType]

        if startingRadius > 0:
            previousDirection = currentRadii[currentAtomType] < startingRadius
            currentRadii[currentAtomType] = startingRadius
        else:
            currentRadii[currentAtomType] = currentRadii[currentAtomType] + radiusIncrement if bestPenalties[currentAtomType] < 0 else currentRadii[currentAtomType] - radiusIncrement
            previousDirection = bestPenalties[currentAtomType] < 0

        numAccepted = 0
        numRejected = 0
        estimatedRadiusIncrement = {t: 0 for t in currentRadii.keys()}
        trace = []
        while True:
            # (sizes / maxSize are those of the LAST evaluation, accepted or not)
            log("Testing ", currentAtomType, ": starting radius=", previousRadius, ", new radius=", currentRadii[currentAtomType],
                ", current weighted penalty=", bestPenalties[currentAtomType] * sizes[currentAtomType] / maxSize,
                ", current median difference=", bestMedianDiffs[currentAtomType], str("(") + str(bestMedianDiffs[currentAtomType]) + str(")"),
                ", size=", sizes[currentAtomType])
            log("Calculating next  median differences: start-time=", str(datetime.datetime.now()), ", current increment=", radiusIncrement)

            (medianDiffs, meanDiffs, overallStdDevDiffs, slopes, sizes, overlapCompleteness), _ = \
                evaluator.iteration({**params, "radii": dict(currentRadii), "slopes": dict(currentSlopes)})
            maxOverlapCompleteness = max(overlapCompleteness.values())
            penalties = optimizeSweep.penalties(medianDiffs, overlapCompleteness, inversePenaltyWeight)

            maxSize = max([sizes[t] for t in medianDiffs.keys() if not atomTypes2Optimize or t in atomTypes2Optimize])
            log("Radii:", currentRadii)
            log("Median Diffs:", medianDiffs)
            log("Overlap Completeness:", overlapCompleteness)
            log("Penalties:", penalties)
            log("Slopes:", slopes)
            _summary(log, medianDiffs, meanDiffs, overallStdDevDiffs, penalties, sizes, maxSize, maxOverlapCompleteness, atomTypes2Optimize)

            step = {"atomType": currentAtomType, "previousRadius": previousRadius, "radius": currentRadii[currentAtomType],
                    "increment": radiusIncrement, "penalty": penalties[currentAtomType], "bestPenalty": bestPenalties[currentAtomType],
                    "medianDiffs": dict(medianDiffs), "penalties": dict(penalties)}
            improved = False
            # Quirk (ref 249): computed from the estimate as it was BEFORE this step's accept / reject updates it.
            directionChangeByIncrement = (previousDirection != (penalties[currentAtomType] < 0)) and estimatedRadiusIncrement[currentAtomType] == 0
            if abs(penalties[currentAtomType]) <= abs(bestPenalties[currentAtomType]):
                numAccepted += 1
                if abs(penalties[currentAtomType]) < abs(bestPenalties[currentAtomType]):
                    # (ref 253: the secant estimate from the best penalty as it was before this step is accepted)
                    estimatedRadiusIncrement[currentAtomType] = 0.9 * (currentRadii[currentAtomType] - previousRadius) * penalties[currentAtomType] / (bestPenalties[currentAtomType] - penalties[currentAtomType])
                    if abs(estimatedRadiusIncrement[currentAtomType]) < minRadiusIncrement:
                        estimatedRadiusIncrement[currentAtomType] = 0
                else:
                    estimatedRadiusIncrement[currentAtomType] = 0
                bestMedianDiffs = medianDiffs
                bestPenalties = penalties
                currentSlopes = {**slopes, **currentSlopes}          # quirk (ref 260): the current slopes win
                # Quirk (ref 261): compared AFTER bestPenalties = penalties, so an accepted step always has improved == 2.
                improved = True if abs(penalties[currentAtomType]) < abs(bestPenalties[currentAtomType]) else 2

                log("Accepted", currentAtomType, ": new radius=", currentRadii[currentAtomType],
                    ", current weighted penalty=", bestPenalties[currentAtomType] * sizes[currentAtomType] / maxSize,
                    ", current weighted median difference=", bestMedianDiffs[currentAtomType] * sizes[currentAtomType] / maxSize,
                    str("(") + str(bestMedianDiffs[currentAtomType]) + str(")"), ", size=", sizes[currentAtomType])
                if rank == 0 and outParamsPath:
                    try:                                              # ref 270-274: a failed temp write does not end the run
                        writeParams(outParamsPath + ".temp", {**params, "radii": currentRadii, "slopes": currentSlopes})
                    except OSError as exception:
                        print('unable to create temporary params file "%s.temp": %s' % (outParamsPath, exception), file=sys.stderr)
            else:
                numRejected += 1
                estimatedRadiusIncrement[currentAtomType] = 0
                log("Rejected", currentAtomType, ": new radius=", currentRadii[currentAtomType])
                currentRadii[currentAtomType] = previousRadius
            step["accepted"] = improved is not False
            trace.append(step)

            testBestPenalties = {t: diff for (t, diff) in bestPenalties.items() if t in atomTypes2Optimize} if atomTypes2Optimize else bestPenalties
            if unweighted:
                maxAtomType = max(testBestPenalties, key=lambda y: abs(testBestPenalties[y]))
            else:
                maxAtomType = max(testBestPenalties, key=lambda y: abs(testBestPenalties[y]) * sizes[y])

            # Keep the order of operations of ref 288 (value * size / maxSize): radii match the reference to the bit.
            if stoppingFractionalDifference > 0 and max([abs(value * sizes[t] / maxSize) for t, value in testBestPenalties.items()]) < stoppingFractionalDifference:
                break

            if maxAtomType == currentAtomType:
                if not improved or previousDirection != (bestPenalties[currentAtomType] < 0):
                    if radiusIncrement == minRadiusIncrement:
                        break

                    radiusIncrement = radiusIncrement / 2.0
                    if radiusIncrement < minRadiusIncrement:
                        radiusIncrement = minRadiusIncrement
                elif improved == 2:
                    radiusIncrement = radiusIncrement * 1.5
                    if radiusIncrement > maxRadiusIncrement:
                        radiusIncrement = maxRadiusIncrement

            elif directionChangeByIncrement:
                radiusIncrement = radiusIncrement * 0.9
                if radiusIncrement < minRadiusIncrement:
                    break

            if maxIterations is not None and len(trace) >= int(maxIterations):
                break                                                 # (not in the reference: the cap for time-limited runs)

            currentAtomType = maxAtomType
            previousRadius = currentRadii[currentAtomType]
            if abs(estimatedRadiusIncrement[currentAtomType]) > 0:
                currentRadii[currentAtomType] = currentRadii[currentAtomType] + estimatedRadiusIncrement[currentAtomType]
            else:
                currentRadii[currentAtomType] = currentRadii[currentAtomType] + radiusIncrement if bestPenalties[currentAtomType] < 0 else currentRadii[currentAtomType] - radiusIncrement
            previousDirection = bestPenalties[currentAtomType] < 0

        log("Final Radii:", currentRadii)
        log("Final Radii Min-Max: [", min(currentRadii.values()), ",", max(currentRadii.values()), "]")
        log("Num Accepted Changes=", numAccepted, ", Num Rejected Changes=", numRejected)
        log("Max Absolute Weighted Median Diff:", max([abs(bestMedianDiffs[t] * sizes[t] / maxSize) for t in bestMedianDiffs.keys() if not atomTypes2Optimize or t in atomTypes2Optimize]))
        log("Max Absolute Weighted Penalty:", max([abs(testBestPenalties[t] * sizes[t] / maxSize) for t in testBestPenalties.keys()]))
        log("Overlap Completeness Min-Max: [", min(overlapCompleteness.values()), ",", max(overlapCompleteness.values()), "]")
        log("Optimization end-time=", str(datetime.datetime.now()))
    finally:
        log.close()

    outParams = {**params, "radii": currentRadii, "slopes": currentSlopes}
    if rank == 0 and outParamsPath:
        writeParams(outParamsPath, outParams)
    return outParams, trace


def sampleEntries(entries, sample=0, seed=None, world_size=1):
    """The reference's ``--sample`` (optimizeParams.py:154-155) drawn with ``random.Random(seed)``; every entry when
    ``sample`` is 0.  Over several ranks the draw needs a ``seed``, or the ranks would draw different samples."""
    entries = list(entries)
    if sample > 0:
        if world_size > 1 and seed is None:
            raise ValueError("sample > 0 over %d ranks needs a seed: every rank must draw the same entries" % world_size)
        entries = random.Random(seed).sample(entries, int(sample))
    return entries


def run(params, entries, *, device=0, workers=4, processes=True, sample=0, seed=None, **optimizeOptions):
    """The whole optimise mode on this rank's GPU: draw ``sample`` entries (``random.Random(seed).sample``, the reference's
    ``--sample``), keep this rank's shard resident (``ProcessSweep`` with ``workers`` processes, or a ``Sweep`` with that many
    streams when ``processes=False``), run ``optimize`` with ``optimizeOptions`` and close the sweep.  Rank and world size come
    from ``torch.distributed`` when a process group is initialised.  Returns what ``optimize`` returns."""
    rank, world_size = _rank_world()
    mine = multipleStructures.shard(sampleEntries(entries, sample, seed, world_size), rank, world_size)
    try:
        sweep = optimizeSweep.ProcessSweep(mine, device, workers) if processes else optimizeSweep.Sweep(mine, device, workers)
    except Exception as exception:
        # the other ranks are about to enter their first evaluation: meet them in its 'ok' exchange so that they raise too
        optimizeStats.all_ranks_ok(exception)
        raise
    try:
        return optimize(params, sweep, **optimizeOptions)
    finally:
        sweep.close()


def compare(params1, params2, name1="params1", name2="params2"):
    """ref optimizeParams.py:67-102 (``--compare``): the lines the reference prints.  A path is loaded and names itself."""
    if not isinstance(params1, dict):
        name1 = params1
    if not isinstance(params2, dict):
        name2 = params2
    params1, params2 = loadParams(params1), loadParams(params2)

    def line(*values):
        return " ".join(str(v) for v in values)

    # (the reference walks a set here; params1's order, then params2's new types, makes the output reproducible)
    atomTypes = list(dict.fromkeys(list(params1["radii"]) + list(params2["radii"])))
    radiusDifferences = {t: params1["radii"][t] - params2["radii"][t] for t in atomTypes
                         if t in params1["radii"] and not np.isnan(params1["radii"][t]) and t in params2["radii"] and not np.isnan(params2["radii"][t])}
    maxRadiusDiffAtomType = max(radiusDifferences, key=lambda y: abs(radiusDifferences[y]))
    meanRadiusDifference = np.nanmean(list(radiusDifferences.values()))
    StDRadiusDifferences = np.nanstd(list(radiusDifferences.values()))
    out = [line("Radii Comparison:", name1, "vs", name2),
           line("Max Radius Difference:", radiusDifferences[maxRadiusDiffAtomType], "for", maxRadiusDiffAtomType, ", leaving_atom =",
                maxRadiusDiffAtomType in params1.get("leaving_atoms", ())),
           line("Mean (Std) Radius Differences:", meanRadiusDifference, str("(") + str(StDRadiusDifferences) + ")")]
    for name, table, what in ((name1, params1["radii"], "radius"), (name2, params2["radii"], "radius"),
                              (name1, params1["slopes"], "slope"), (name2, params2["slopes"], "slope")):
        nanAtomTypes = [t for (t, v) in table.items() if np.isnan(v)]
        if nanAtomTypes:
            out.append(line("AtomTypes in", name, "with NaN %s:" % what, ", ".join(nanAtomTypes)))
    return out


def finalize(params):
    """ref optimizeParams.py:103-117 (``--finalize``): the table for general use -- without its ``optimize`` list.
    Write it with ``writeParams``."""
    params = loadParams(params)
    params.pop("optimize", None)
    return params


class MirrorEntryLoader(object):
    """Loader of one entry of a local mirror laid out like ``densityAnalysis.fromPDBid`` (``<ccp4folder><id>.ccp4``,
    ``<id>_diff.ccp4``, ``<pdbfolder>pdb<id>.ent.gz``).  The maps go as PATHS (file -> HBM); picklable for worker processes."""

    def __init__(self, pdbid, ccp4folder, pdbfolder):
        self.pdbid = pdbid.lower()
        self.density_path = os.path.abspath(ccp4folder + self.pdbid + ".ccp4")
        self.diff_path = os.path.abspath(ccp4folder + self.pdbid + "_diff.ccp4")
        self.pdb_path = os.path.abspath(pdbfolder + "pdb" + self.pdbid + ".ent.gz")

    def __call__(self):
        from . import structure
        biopdbObj, pdbObj = structure.read_pdb(self.pdb_path, self.pdbid)
        return self.density_path, self.diff_path, biopdbObj, pdbObj


def entriesFromPDBids(pdbids):
    """``multipleStructures.Entry`` objects for PDB ids of the local mirror (``densityAnalysis.ccp4folder`` / ``pdbfolder``,
    ``./ccp4_data`` and ``./pdb_data`` by default).  The cost hint is the 2Fo-Fc map's size, so sharding deals the biggest first."""
    out = []
    for pdbid in pdbids:
        loader = MirrorEntryLoader(pdbid, densityAnalysis.ccp4folder, densityAnalysis.pdbfolder)
        try:
            cost = os.path.getsize(loader.density_path)
        except OSError:
            cost = 0.0
        out.append(multipleStructures.Entry(loader.pdbid, loader, cost_hint=cost))
    return out
