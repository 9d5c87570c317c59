"""The maps and taps of the filter tests (shared by tests/test_filter_host.py and tests/test_gpu_filter.py): seeded, so both see the same
numbers.  The geometries box, skew and rep are those of tests/model_cases.py; the others exist for the kernels' work units.  The data are
smoothed noise plus an offset, so local means are not about 0 and a wrong normalisation shows."""
import io

import numpy as np

from pdb_eda_amd import ccp4, synthetic

import model_cases

UNIT_C = (64, 4)            # FC_RUN, FC_ROWS of pdb_eda_amd/csrc/pdbeda_filter.h: outputs along c x rows of one workgroup of the pass along c
UNIT_LINE = (32, 32)        # FL_LANES, FL_CHUNK: columns x outputs along the filtered axis of one workgroup of a pass along r or s
MAX_RADIUS = 64             # PDBEDA_FILTER_MAX_RADIUS
gaussianTaps, boxTaps = ccp4.gaussianTaps, ccp4.boxTaps          # (looked up on import: without the feature neither test module loads)

SPECS = dict((name, model_cases.SPECS[name]) for name in ("box", "skew", "rep"))
SPECS.update({
    "unit": dict(ncrs=(UNIT_C[0], UNIT_LINE[1], UNIT_LINE[1]), spacing=0.5),                   # exactly one work unit of every pass along every axis (two columns of lanes)
    "past": dict(ncrs=(UNIT_C[0] + 1, UNIT_LINE[1] + 1, UNIT_LINE[1] + 1), spacing=0.5),       # one voxel past it
    "lanes": dict(ncrs=(UNIT_LINE[0], UNIT_C[1], 1), spacing=0.5),                             # one column tile of a line pass, one workgroup of rows
    "lanes_past": dict(ncrs=(UNIT_LINE[0] + 1, UNIT_C[1] + 1, 1), spacing=0.5),
    "line": dict(ncrs=(70, 1, 1), spacing=0.5),                                                # radius 64 wraps a 70-voxel line once
    "cut": dict(ncrs=(70, 3, 2), interval=(100, 3, 2), spacing=0.5),                           # the same line as a cut-out of a 100-step cell
})
_headers, _grids = {}, {}


def spec_of(name):
    return synthetic.MapSpec(**SPECS[name])


def header_of(name):
    if name not in _headers:
        spec = spec_of(name)
        nc, nr, ns = spec.ncrs
        _headers[name] = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((ns, nr, nc), dtype=np.float32))))[0]
    return _headers[name]


def intervals_of(name):
    return [int(v) for v in header_of(name).crsInterval]


def grid_of(name, seed=0, offset=1.5):
    """Smoothed noise of unit scale plus ``offset``, float32 [s][r][c]."""
    key = (name, seed, offset)
    if key not in _grids:
        nc, nr, ns = spec_of(name).ncrs
        g = synthetic.smooth_noise((ns, nr, nc), 100 + seed, 1.0).astype(np.float64)
        g = g / max(float(g.std()), 1e-6) + offset
        _grids[key] = np.ascontiguousarray(g, dtype=np.float32)
        _grids[key].setflags(write=False)
    return _grids[key]


def asymmetric(radius, seed=7):
    """Positive taps without any symmetry: a reversed window gives other numbers."""
    rng = np.random.default_rng(seed + radius)
    w = rng.uniform(0.1, 1.0, size=2 * radius + 1) * np.linspace(0.2, 1.8, 2 * radius + 1)
    return w / w.sum()


def signed(radius, seed=3):
    """Taps of both signs (a derivative-like kernel), not for renormalisation."""
    rng = np.random.default_rng(seed + radius)
    return rng.uniform(-1.0, 1.0, size=2 * radius + 1)


def one_sided(radius):
    """Zeros at the low end, weight only on the neighbours at i + 1 .. i + radius: at the high face of a cut-out nothing is met, N = 0."""
    w = np.zeros(2 * radius + 1)
    w[radius + 1:] = 1.0 / radius
    return w


def tap_sets():
    """name -> (taps_c, taps_r, taps_s)."""
    g = ccp4.gaussianTaps
    return {
        "gauss": (g(1.5), g(0.8), g(0.4, 3.0)),                      # radii 6, 3, 1
        "asym": (asymmetric(4), asymmetric(2), asymmetric(3)),
        "signed": (signed(3), signed(1), signed(2)),
        "identity": (np.ones(1), np.ones(1), np.ones(1)),
        "wrap24": (g(6.0), asymmetric(1), g(0.5)),                   # radius 24 on the 21-voxel axis
        "box": (ccp4.boxTaps(2), ccp4.boxTaps(1), ccp4.boxTaps(1)),
        "one_sided": (one_sided(2), ccp4.boxTaps(1), one_sided(1)),
        "r64": (g(16.0), np.ones(1), np.ones(1)),                    # radius 64
    }
