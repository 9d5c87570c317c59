"""bench.py's host-side helpers that need no GPU: the CPU share of the cgroup, the carried phantom-ranks table, the algorithmic bytes,
the output dump and the options of a plain run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_cpu_share_is_the_quota_or_the_mask():
    import bench
    cores, affinity, quota = bench.cpu_share()
    assert 1 <= cores <= affinity == len(os.sched_getaffinity(0))
    if quota is not None:
        assert cores == max(1, min(affinity, int(quota + 0.5)))
    else:
        assert cores == affinity


def test_host_contention_carries_the_committed_runs():
    import bench
    hc = bench.host_contention()
    assert hc is not None and hc["rows"], "profiles/r*_phantom_ranks_*.json are committed"
    base = [r for r in hc["rows"] if r["phantom_ranks"] == 0]
    assert base and all(r["both_maps_k_per_min"] > 0 and r["lazy_k_per_min"] > 0 for r in hc["rows"])
    assert "quota" in hc["note"]
    json.dumps(hc)      # (goes into the bench line)


def test_algorithmic_bytes_of_the_labelling_pass():
    import bench
    n = 256 ** 3
    assert bench.algorithmic_bytes("k_tile_label", n, 2) == 4 * n + 12 * (n // 64) * 2
    assert bench.algorithmic_bytes("k_labels_tiles", n, 2) == bench.algorithmic_bytes("k_tile_label", n, 2)
    assert not bench.algorithmic_bytes("k_face_merge", n, 2)


class _FakeBlobList(object):
    """What dump_outputs reads of a BlobList: stats(), voxels(), labels(shape)."""

    def __init__(self, n_blobs, n_voxels, shape, seed, sign):
        import numpy as np
        rng = np.random.default_rng(seed)
        self._stats = {"n": rng.integers(1, 50, n_blobs), "totalDensity": rng.standard_normal(n_blobs), "centroid": rng.standard_normal((n_blobs, 3)),
                       "coordCenter": rng.standard_normal((n_blobs, 3)), "volume": rng.random(n_blobs), "firstKey": np.arange(n_blobs, dtype=np.int64) * 7,
                       "group": np.zeros(n_blobs, np.int32)}
        self._crs = rng.integers(0, 256, (n_voxels, 3)).astype(np.int32)
        self._off = np.linspace(0, n_voxels, n_blobs + 1).astype(np.int64)
        self._labels = (sign * rng.integers(0, n_blobs + 1, int(np.prod(shape)))).astype(np.int32)

    def stats(self):
        return self._stats

    def voxels(self):
        return self._crs, self._off

    def shuffled_inside_blobs(self, seed):
        """The same blobs with every blob's voxels in another order (the device's tiles may emit them so)."""
        import copy
        import numpy as np
        rng = np.random.default_rng(seed)
        other = copy.copy(self)
        other._crs = self._crs.copy()
        for i in range(len(self._off) - 1):
            a, b = self._off[i], self._off[i + 1]
            other._crs[a:b] = self._crs[a:b][rng.permutation(b - a)]
        return other

    def labels(self, shape):
        return self._labels.reshape(shape)


def test_dump_outputs_is_seeded_typed_and_bounded(tmp_path):
    import numpy as np
    import bench
    shape = (128, 128, 64)
    green = _FakeBlobList(bench.DUMP_BLOBS + 5, bench.DUMP_VOXELS + 7, shape, 1, 1)
    red = _FakeBlobList(300, 4000, shape, 2, -1)
    first = bench.dump_outputs(str(tmp_path / "a"), green, red, shape, True)
    again = bench.dump_outputs(str(tmp_path / "b"), green, red, shape, True)
    assert first == again
    total = 0
    for name in first:
        a, b = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT
    assert first["green_n"] == [bench.DUMP_BLOBS] and first["green_centroid"] == [bench.DUMP_BLOBS, 3] and first["red_n"] == [300]
    assert first["green_voxels_crs"] == [bench.DUMP_VOXELS, 3] and first["red_voxels_crs"] == [4000, 3]
    assert first["green_labels_sample"] == first["red_labels_sample"] == first["labels_sample_index"] == [bench.DUMP_LABELS]
    # the sampled rows are rows of the source, in order; small arrays are whole
    key = np.load(str(tmp_path / "a" / "green_firstKey.npy"))
    assert (np.diff(key) > 0).all() and (key % 7 == 0).all()
    assert np.array_equal(np.load(str(tmp_path / "a" / "red_voxels_crs.npy")), bench.canonical_voxels(*red.voxels()).astype(np.float32))
    where = np.load(str(tmp_path / "a" / "labels_sample_index.npy")).astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "a" / "red_labels_sample.npy")), red.labels(shape).reshape(-1)[where])
    plain = bench.dump_outputs(str(tmp_path / "c"), green, red, shape, False)
    assert not any("labels" in name for name in plain)
    # the order of the voxels inside a blob is not part of the result
    bench.dump_outputs(str(tmp_path / "d"), green.shuffled_inside_blobs(5), red.shuffled_inside_blobs(6), shape, True)
    for name in first:
        assert np.array_equal(np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "d" / (name + ".npy")))), name


def test_canonical_voxels_sorts_inside_blobs_only():
    import numpy as np
    import bench
    crs = np.array([[5, 0, 0], [1, 2, 3], [1, 2, 0], [9, 9, 9], [0, 0, 0], [3, 1, 1]], dtype=np.int32)
    off = np.array([0, 3, 4, 6], dtype=np.int64)
    want = np.array([[1, 2, 0], [1, 2, 3], [5, 0, 0], [9, 9, 9], [0, 0, 0], [3, 1, 1]], dtype=np.int32)
    assert np.array_equal(bench.canonical_voxels(crs, off), want)


def test_plain_run_is_the_default(monkeypatch):
    import pytest
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse_args()
    assert not args.full and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert args.full and args.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
