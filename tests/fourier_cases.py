"""The maps of the Fourier tests (shared by tests/test_fourier_host.py and tests/test_gpu_fourier.py): seeded, so both see the same numbers.
The data are smoothed noise plus an offset, as tests/filter_cases.py makes them, so F(000) is large and every shell holds power.  Shapes are
(nc, nr, ns), the smallest at which the transform kernels can still go wrong; the harness helpers build and run tests/fourier_harness.cpp."""
import io
import os
import re
import subprocess

import numpy as np

from pdb_eda_amd import ccp4, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pdb_eda_amd", "csrc")
fourierSize, reciprocalMetric, shellEdges = ccp4.fourierSize, ccp4.reciprocalMetric, ccp4.shellEdges      # (looked up on import: without the feature no test module loads)


def _unit():
    """FFT_LINES of pdb_eda_amd/csrc/pdbeda_fourier.h: the lines of a tile, which is both the rows of a workgroup of the passes along c (R)
    and the half-spectrum columns of a workgroup of the strided passes (T)."""
    text = open(os.path.join(CSRC, "pdbeda_fourier.h")).read()
    lines = int(re.search(r"constexpr int FFT_LINES = (\d+);", text).group(1))
    assert "constexpr int FFT_ROWS = FFT_LINES;" in text and "constexpr int FFT_COLS = FFT_LINES;" in text
    return lines, lines


T, R = _unit()
MAX_AXIS = 1024      # PDBEDA_FFT_MAX_AXIS

SPECS = {
    "one": dict(ncrs=(1, 1, 1), spacing=0.5),                                      # n = 1: no pass at all
    "r235": dict(ncrs=(2, 3, 5), spacing=0.5),                                     # every radix alone
    "r753": dict(ncrs=(7, 5, 3), spacing=0.5),                                     # all axes odd: no Nyquist column
    "p4": dict(ncrs=(4, 4, 4), spacing=0.5),                                       # one radix-4 butterfly a line
    "p64": dict(ncrs=(64, 64, 64), spacing=0.5),                                   # a power of two, three radix-4 passes
    "mixed": dict(ncrs=(30, 36, 70), spacing=0.5),                                 # 2 3 5 / 4 3 3 / 2 5 7
    "hex": dict(ncrs=(30, 36, 70), cell=(15.0, 18.0, 35.0), angles=(90.0, 90.0, 120.0)),
    "perm": dict(ncrs=(30, 36, 70), axis_order=(2, 3, 1), spacing=0.5),             # columns along y, rows along z, sections along x
    "mid": dict(ncrs=(48, 48, 50), spacing=0.5),                                   # 115 200 voxels
    "longc": dict(ncrs=(MAX_AXIS, 3, 2), spacing=0.5),                             # the longest line on every axis
    "longr": dict(ncrs=(3, MAX_AXIS, 2), spacing=0.5),
    "longs": dict(ncrs=(2, 3, MAX_AXIS), spacing=0.5),
    "tile_past": dict(ncrs=(T + 1, R + 1, 2), spacing=0.5),                        # one row past the rows of a workgroup
    "cols_past": dict(ncrs=(2 * T, R + 1, 3), spacing=0.5),                        # T + 1 half-spectrum columns: one past the column tile
    "cut": dict(ncrs=(30, 36, 70), interval=(60, 72, 140), crs_start=(5, -3, 11), spacing=0.5),      # a cut-out: the box, not the cell, is the period
}
FORWARD = ("one", "r235", "r753", "p4", "p64", "mixed", "hex", "perm", "longc", "longr", "longs", "tile_past", "cols_past")
GEOMETRIES = ("mixed", "hex", "perm", "cut")
FILTER_MAPS = ("mid", "mixed", "p64")        # 115 200, 75 600 and 262 144 voxels
_headers, _grids = {}, {}


def spec_of(name):
    return synthetic.MapSpec(**SPECS[name])


def header_of(name):
    if name not in _headers:
        spec = spec_of(name)
        nc, nr, ns = spec.ncrs
        _headers[name] = ccp4.read_grid(io.BytesIO(synthetic.ccp4_bytes(spec, np.zeros((ns, nr, nc), dtype=np.float32))))[0]
    return _headers[name]


def shape_of(name):
    nc, nr, ns = spec_of(name).ncrs
    return (ns, nr, nc)


def grid_of(name, seed=0, offset=1.5):
    """Smoothed noise of unit scale plus ``offset``, float32 [s][r][c] (read-only)."""
    key = (name, seed, offset)
    if key not in _grids:
        shape = shape_of(name)
        sigma = [min(1.0, 0.25 * n) for n in shape]
        rng = np.random.default_rng(4100 + seed)
        from scipy.ndimage import gaussian_filter
        g = gaussian_filter(rng.standard_normal(shape), sigma=sigma, mode="wrap")
        g = g / max(float(g.std()), 1e-6) + offset
        _grids[key] = np.ascontiguousarray(g, dtype=np.float32)
        _grids[key].setflags(write=False)
    return _grids[key]


def filters(header):
    """name -> (table, s2Max, beyond): a B-factor blur, a sharpening and a soft 3 A cut."""
    s2max = ccp4.maxS2(header)
    cut = ccp4.resolutionTable(3.0, None, 0.2)
    return {
        "blur": (ccp4.bFactorTable(20.0, s2max), s2max, 0.0),
        "sharpen": (ccp4.bFactorTable(-8.0, s2max), s2max, 0.0),
        "cut3": (cut, ((1.0 + 0.1) / 3.0) ** 2 * (1.0 + 2.0 ** -20), 0.0),
    }


def edges_of(name, n_shells=12):
    return ccp4.shellEdges(header_of(name), n_shells)


# ---- tests/fourier_harness.cpp ---------------------------------------------------------------------------------------------------
def build_harness(directory, sanitize):
    """The harness built with the host compiler; under ASan + UBSan (nothing recovered, nothing preloaded) when ``sanitize``."""
    exe = os.path.join(str(directory), "fourier_harness_san" if sanitize else "fourier_harness")
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-g", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off"] + flags + ["-I" + CSRC, os.path.join(ROOT, "tests", "fourier_harness.cpp"), "-o", exe])
    return exe


def harness_volume(exe, directory, grid, tag):
    """The half spectrum of ``grid`` by the harness: complex128 [ns][nr][nc // 2 + 1]."""
    ns, nr, nc = grid.shape
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.array([nc, nr, ns], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(grid, dtype=np.float32).tobytes())
    proc = subprocess.run([exe, "volume", src, dst], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0 and proc.stderr == "", (proc.returncode, proc.stderr[-2000:])
    return np.fromfile(dst, dtype=np.complex128).reshape(ns, nr, nc // 2 + 1)


def harness_lines(exe, directory, lines, tag="lines"):
    """[(forward, inverse, twiddles)] of complex128 lines by the harness; the run's CompletedProcess comes last."""
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.array([len(lines)], dtype=np.int32).tobytes())
        for x in lines:
            f.write(np.array([len(x)], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(x, dtype=np.complex128).tobytes())
    proc = subprocess.run([exe, "lines", src, dst], capture_output=True, text=True, timeout=300)
    if proc.returncode != 0:
        return [], proc
    raw = np.fromfile(dst, dtype=np.complex128)
    out, at = [], 0
    for x in lines:
        n = len(x)
        out.append((raw[at:at + n], raw[at + n:at + 2 * n], raw[at + 2 * n:at + 3 * n]))
        at += 3 * n
    assert at == len(raw)
    return out, proc
