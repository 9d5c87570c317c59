"""A deterministic stand-in for one optimise-mode evaluation: medians, sizes and overlap completeness as smooth functions of the
radii, so the descent's decisions can be replayed without analysing any map.

Shared by tests/golden/make_golden_optimize.py (it replaces the reference's ``calculateMedianDiffsSlopes``) and the descent
tests (``Surface`` is an evaluator for ``optimizeParams.optimize``): both sides see the same numbers to the bit.

Per atom type t (index i in ``params["radii"]`` order):
  * median diff   a_i (r_t - r*_t) + c sum_{s != t} (r_s - r*_s)      (linear, small cross terms; quantised by ``flat``)
  * completeness  1 / (1 + exp(-k (r_t - r0_t)))                     (logistic in the radius)
  * size          fixed per type
"""
import math

TARGET_SHIFT = (0.11, -0.07, 0.16, -0.13, 0.05, -0.19)
GAIN = (0.9, 1.3, 0.7, 1.1, 1.6, 0.8)
SIZE = (40, 25, 40, 12, 31, 7)


def surface_params():
    """A small parameter table for the surface (made-up values, the schema of the reference's params file)."""
    types = ["N.srf.amide", "C.srf.alpha", "C.srf.carbonyl", "O.srf.carbonyl", "C.srf.methyl", "S.srf.thiol"]
    radii = [0.78, 0.81, 0.74, 0.86, 0.9, 1.02]
    slopes = [-0.52, -0.61, -0.55, -0.48, -0.7, -0.33]
    return {"radii": dict(zip(types, radii)), "slopes": dict(zip(types[:5], slopes[:5])),
            "bonded_atoms": {}, "full_atom_name_map_atom_type": {}, "full_atom_name_map_electrons": {},
            "leaving_atoms": ["O.srf.carbonyl"]}


class Surface(object):
    """``iteration(params)`` -> ((medianDiffs, meanDiffs, overallStdDevDiffs, medianSlopes, sizes, overlapCompleteness), records),
    the evaluator interface of ``optimizeParams.optimize``; ``reduction(params)`` is the tuple alone (what the reference's
    ``calculateMedianDiffsSlopes`` returns).  ``flat`` > 0 quantises the medians and completeness into steps of that width in the
    radius, so neighbouring radii give EQUAL penalties."""

    def __init__(self, base, flat=0.0, cross=0.03, steepness=6.0):
        self.types = list(base["radii"])
        self.target = {t: base["radii"][t] + TARGET_SHIFT[i % len(TARGET_SHIFT)] for i, t in enumerate(self.types)}
        self.mid = {t: base["radii"][t] - 0.05 * (i % 3) for i, t in enumerate(self.types)}
        self.gain = {t: GAIN[i % len(GAIN)] for i, t in enumerate(self.types)}
        self.size = {t: SIZE[i % len(SIZE)] for i, t in enumerate(self.types)}
        self.flat, self.cross, self.steepness = flat, cross, steepness
        self.calls = 0

    def _q(self, x):
        return math.floor(x / self.flat) * self.flat if self.flat > 0 else x

    def reduction(self, params):
        self.calls += 1
        radii = params["radii"]
        dev = {t: self._q(radii[t] - self.target[t]) for t in self.types}
        total = sum(dev.values())
        median = {t: self.gain[t] * dev[t] + self.cross * (total - dev[t]) for t in self.types}
        mean = {t: median[t] + 0.01 * (i + 1) for i, t in enumerate(self.types)}
        std = math.sqrt(sum(v * v for v in median.values()) / (len(median) - 1))
        slopes = {t: -0.5 - 0.1 * radii[t] for t in self.types}
        completeness = {t: 1.0 / (1.0 + math.exp(-self.steepness * self._q(radii[t] - self.mid[t]))) for t in self.types}
        return median, mean, std, slopes, dict(self.size), completeness

    def iteration(self, params):
        return self.reduction(params), []


# the option sets of golden Case A: (name, surface keywords, changes to the start table, optimize() keywords)
CASES = [
    ("default", {}, {}, {}),
    ("unweighted", {}, {}, {"unweighted": True}),
    ("start_radius", {}, {}, {"startAtomType": "C.srf.carbonyl", "startRadius": 0.95}),
    ("stop", {}, {}, {"stop": 0.05, "inversePenaltyWeight": 2.0}),
    ("optimize_list", {}, {"optimize": ["C.srf.alpha", "O.srf.carbonyl", "S.srf.thiol"]}, {}),
    ("optimize_reverse", {}, {"optimize": ["C.srf.alpha", "O.srf.carbonyl", "S.srf.thiol"]}, {"reverse": True}),
    ("ignore", {}, {"optimize": ["C.srf.alpha"]}, {"ignore": True, "maxIncrement": 0.1}),
    ("small_min", {}, {}, {"maxIncrement": 0.05, "minIncrement": 1e-5}),
    ("flat", {"flat": 0.05}, {}, {"maxIncrement": 0.1, "minIncrement": 0.004}),
]
