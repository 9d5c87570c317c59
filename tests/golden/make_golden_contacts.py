"""Golden vectors for crystal contacts: the REFERENCE's crystalContacts.findCoordContacts (crystalContacts.py:87-101, scipy
cdist + np.min) on seeded coordinate sets.  Build container only:
    python tests/golden/make_golden_contacts.py   -> tests/golden/contacts_ref.npz
The module is imported through refload's package stub; ``docopt`` is stubbed (the command line is not used) and pymol is
absent, which the module tolerates at import.  Cases: 300 x 2 000 random points; integer points at distances of exactly 5.0
(3-4-5 triangles) and just beyond; duplicate points (in either list, and queries that coincide with a neighbour)."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

CUTOFF = 5.0


def cases():
    rng = np.random.default_rng(20261016)
    out = {}
    out["random"] = (rng.uniform(0.0, 60.0, (300, 3)), rng.uniform(-5.0, 65.0, (2000, 3)))
    # exact boundary: each query has its nearest neighbour at an integer offset of length exactly 5 (or 5 + a little, 4.9 ...)
    base = rng.integers(-40, 40, (60, 3)).astype(np.float64) * 20.0
    offs = np.array([[3, 4, 0], [0, 3, 4], [4, 0, 3], [5, 0, 0], [0, 0, -5], [-3, -4, 0], [3, 4, 1], [0, 5, 1], [2, 4, 4], [0, 3, 3]], dtype=np.float64)
    q = base
    p = base + offs[np.arange(len(base)) % len(offs)]
    out["boundary"] = (q, np.concatenate([p, base[:5] + 100.0]))
    # duplicates: repeated query points, repeated neighbour points, queries sitting on a neighbour (distance 0)
    pts = rng.uniform(0.0, 20.0, (80, 3))
    q = np.concatenate([pts[:40], pts[:40], pts[70:]])
    p = np.concatenate([pts[30:60], pts[30:60], pts[65:75] + 0.5])
    out["duplicates"] = (q, p)
    return out


def main():
    refload.load(with_density_analysis=True)
    pkg = sys.modules["pdb_eda"]
    pkg.__version__ = "reference"
    if "docopt" not in sys.modules:
        sys.modules["docopt"] = types.ModuleType("docopt")
    cc = importlib.import_module("pdb_eda.crystalContacts")
    arrays = {"cutoff": np.float64(CUTOFF)}
    for name, (q, p) in cases().items():
        got = cc.findCoordContacts(q, p, CUTOFF)
        arrays[name + "_q"] = q
        arrays[name + "_p"] = p
        arrays[name + "_index"] = np.array([i for i, _ in got], dtype=np.int64)
        arrays[name + "_distance"] = np.array([float(d) for _, d in got], dtype=np.float64)
        print(name, len(q), len(p), "->", len(got), "contacts")
    path = os.path.join(HERE, "contacts_ref.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
