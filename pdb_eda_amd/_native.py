"""ctypes binding of ``libpdbeda_hip.so`` (C-ABI in ``include/pdbeda.h``).

This is the reference-side stub a pdb_eda maintainer would add:
plain pointers and sizes, no torch types.  There is deliberately NO fallback: if the
shared library is missing, or no gfx950 device is usable, every operation raises.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDBEDA_LIB") or os.path.join(_HERE, "libpdbeda_hip.so")   # PDBEDA_LIB: A/B builds of the same library

PDBEDA_FLAG_LABELS = 1


class PdbedaError(RuntimeError):
    """A device / library failure (never an entry-level condition): callers must not swallow it."""


class PdbedaTimeout(PdbedaError):
    """The per-entry watchdog of a context expired (PDBEDA_ERR_TIMEOUT): that context is abandoned."""


PDBEDA_ERR_TIMEOUT = -6
PDBEDA_ERR_ARGUMENT = -2


class Geometry(C.Structure):
    _fields_ = [("ncrs", C.c_int32 * 3), ("crs_start", C.c_int32 * 3), ("xyz_interval", C.c_int32 * 3),
                ("map2xyz", C.c_int32 * 3), ("map2crs", C.c_int32 * 3), ("orthogonal", C.c_int32),
                ("ortho", C.c_double * 9), ("deortho", C.c_double * 9), ("origin", C.c_double * 3),
                ("grid_len", C.c_double * 3), ("unit_volume", C.c_double)]


class CloudAtoms(C.Structure):
    """pdbeda_cloud_atoms (include/pdbeda.h): the flattened input of pdbeda_aggregate_cloud."""
    _fields_ = [("n", C.c_int64), ("xyz", C.c_void_p), ("radius", C.c_void_p), ("weight", C.c_void_p), ("residue", C.c_void_p),
                ("alias", C.c_void_p), ("key", C.c_void_p), ("n_keys", C.c_int64), ("bonded_off", C.c_void_p), ("bonded", C.c_void_p),
                ("n_owners", C.c_int64), ("owner_key", C.c_void_p)]


def make_geometry(ncrs, crs_start, xyz_interval, map2xyz, map2crs, orthogonal, ortho, deortho, origin, grid_len, unit_volume):
    g = Geometry()
    for k in range(3):
        g.ncrs[k] = int(ncrs[k])
        g.crs_start[k] = int(crs_start[k])
        g.xyz_interval[k] = int(xyz_interval[k])
        g.map2xyz[k] = int(map2xyz[k])
        g.map2crs[k] = int(map2crs[k])
        g.origin[k] = float(origin[k])
        g.grid_len[k] = float(grid_len[k])
    g.orthogonal = 1 if orthogonal else 0
    o = np.asarray(ortho, dtype=np.float64).reshape(9)
    d = np.asarray(deortho, dtype=np.float64).reshape(9)
    for k in range(9):
        g.ortho[k] = float(o[k])
        g.deortho[k] = float(d[k])
    g.unit_volume = float(unit_volume)
    return g


_lib = None
_lib_lock = threading.Lock()

_p = C.c_void_p
_i64 = C.c_int64
_SIGS = {
    "pdbeda_version": (C.c_char_p, []),
    "pdbeda_device_count": (C.c_int, []),
    "pdbeda_device_pci_address": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "pdbeda_ctx_create": (C.c_int, [C.c_int, C.POINTER(_p)]),
    "pdbeda_ctx_create_on_stream": (C.c_int, [C.c_int, _p, C.POINTER(_p)]),
    "pdbeda_ctx_destroy": (C.c_int, [_p]),
    "pdbeda_ctx_synchronize": (C.c_int, [_p]),
    "pdbeda_ctx_stream": (_p, [_p]),
    "pdbeda_ctx_set_timeout": (C.c_int, [_p, C.c_double]),
    "pdbeda_reap_abandoned": (C.c_int64, []),
    "pdbeda_last_error": (C.c_char_p, [_p]),
    "pdbeda_ctx_profile_begin": (C.c_int, [_p]),
    "pdbeda_ctx_profile_end": (C.c_int, [_p, C.c_char_p, _i64]),
    "pdbeda_map_upload": (C.c_int, [_p, _p, C.POINTER(Geometry), C.POINTER(_p)]),
    "pdbeda_map_upload_stats": (C.c_int, [_p, _p, C.POINTER(Geometry), C.POINTER(_p), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pdbeda_map_upload_file": (C.c_int, [_p, C.c_char_p, _i64, C.c_int, C.POINTER(Geometry), C.POINTER(_p)]),
    "pdbeda_map_upload_file_stats": (C.c_int, [_p, C.c_char_p, _i64, C.c_int, C.POINTER(Geometry), C.POINTER(_p), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pdbeda_map_from_device": (C.c_int, [_p, _p, C.POINTER(Geometry), C.POINTER(_p)]),
    "pdbeda_map_invalidate": (C.c_int, [_p]),
    "pdbeda_map_free": (C.c_int, [_p]),
    "pdbeda_map_combine": (C.c_int, [_p, _p, C.c_double, C.POINTER(_p)]),
    "pdbeda_map_download": (C.c_int, [_p, _p]),
    "pdbeda_abs_select_hist": (C.c_int, [_p, _p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, _p]),
    "pdbeda_map_stats": (C.c_int, [_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pdbeda_sum_of_abs": (C.c_int, [_p, C.c_float, C.POINTER(C.c_double)]),
    "pdbeda_point_density": (C.c_int, [_p, _p, _i64, _p]),
    "pdbeda_valid_crs": (C.c_int, [_p, _p, _i64, _p]),
    "pdbeda_crs2xyz": (C.c_int, [_p, _p, _i64, _p]),
    "pdbeda_xyz2crs": (C.c_int, [_p, _p, _i64, _p]),
    "pdbeda_full_blobs": (C.c_int, [_p, C.c_float, C.c_uint32, C.POINTER(_p)]),
    "pdbeda_full_blobs_pm": (C.c_int, [_p, C.c_float, C.c_float, C.c_uint32, C.POINTER(_p), C.POINTER(_p)]),
    "pdbeda_sphere_blobs": (C.c_int, [_p, _p, _p, _i64, _p, _i64, C.c_float, C.POINTER(_p)]),
    "pdbeda_list_blobs": (C.c_int, [_p, _p, _i64, _p, _i64, C.POINTER(_p)]),
    "pdbeda_bloblist_count": (_i64, [_p]),
    "pdbeda_bloblist_num_voxels": (_i64, [_p]),
    "pdbeda_bloblist_stats": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_bloblist_voxels": (C.c_int, [_p, _p, _p]),
    "pdbeda_bloblist_moments": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_bloblist_labels": (C.c_int, [_p, _p]),
    "pdbeda_bloblist_nearest": (C.c_int, [_p, _p, _p, _i64, _p, _p, _p, _p]),
    "pdbeda_bloblist_free": (C.c_int, [_p]),
    "pdbeda_bloblist_counters": (C.c_int, [_p, _p]),
    "pdbeda_map_peaks": (C.c_int, [_p, C.c_float, _p, C.POINTER(_p)]),
    "pdbeda_map_peaks_pm": (C.c_int, [_p, C.c_float, C.c_float, _p, _p, C.POINTER(_p), C.POINTER(_p)]),
    "pdbeda_peaklist_count": (_i64, [_p]),
    "pdbeda_peaklist_rows": (C.c_int, [_p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_peaklist_counters": (C.c_int, [_p, _p]),
    "pdbeda_peaklist_basins": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_peaklist_free": (C.c_int, [_p]),
    "pdbeda_region_sums": (C.c_int, [_p, _p, _p, _i64, _p, _i64, C.c_float, _p, _p, _p, _p]),
    "pdbeda_radial_profiles": (C.c_int, [_p, _p, _i64, C.c_float, C.c_int32, C.c_float, _p, _p, _p, _p, _p]),
    "pdbeda_map_partition": (C.c_int, [_p, _p, _i64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_interp_density": (C.c_int, [_p, _p, _i64, _p, _p]),
    "pdbeda_atom_qscores": (C.c_int, [_p, _p, _i64, _p, _i64, C.c_float, C.c_int32, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p]),
    "pdbeda_model_density": (C.c_int, [_p, _p, _i64, C.c_int32, _p, _p, _p, C.POINTER(_p), _p]),
    "pdbeda_map_pair_moments": (C.c_int, [_p, _p, C.c_float, C.POINTER(_i64), _p]),
    "pdbeda_atom_moments": (C.c_int, [_p, _p, _i64, C.c_int32, _p, _p, C.c_uint32, _p, _p, _p]),
    "pdbeda_pose_scores": (C.c_int, [_p, _p, _p, C.c_int32, _p, _i64, _p, _i64, C.c_float, C.c_int32, C.c_int32, C.c_uint32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "pdbeda_map_filter": (C.c_int, [_p, _p, C.c_int32, _p, C.c_int32, _p, C.c_int32, C.c_uint32, C.POINTER(_p)]),
    "pdbeda_map_local_stats": (C.c_int, [_p, _p, _p, C.c_int32, _p, C.c_int32, _p, C.c_int32, C.c_double, _p, _p, _p, _p, _p, _p]),
    "pdbeda_map_spread": (C.c_int, [_p, C.c_float, C.c_uint32, _p, _i64, _p, _p, C.POINTER(_p), _p]),
    "pdbeda_map_resample": (C.c_int, [_p, C.POINTER(Geometry), _p, C.c_int32, C.c_int32, C.c_uint32, C.c_float, _p, C.c_double, C.POINTER(_p), C.POINTER(_p), _p]),
    "pdbeda_map_fft": (C.c_int, [_p, C.POINTER(_p)]),
    "pdbeda_spectrum_inverse": (C.c_int, [_p, _p, C.POINTER(_p)]),
    "pdbeda_spectrum_shape": (C.c_int, [_p, _p]),
    "pdbeda_spectrum_download": (C.c_int, [_p, _p]),
    "pdbeda_spectrum_free": (C.c_int, [_p]),
    "pdbeda_spectrum_values": (C.c_int, [_p, _p, _i64, _p]),
    "pdbeda_spectrum_scale": (C.c_int, [_p, _p, _p, C.c_int32, C.c_double, C.c_double]),
    "pdbeda_spectrum_shells": (C.c_int, [_p, _p, _p, _p, C.c_int32, _p, _p]),
    "pdbeda_aggregate_cloud": (C.c_int, [_p, C.POINTER(CloudAtoms), C.c_float, C.c_double, C.POINTER(_p)]),
    "pdbeda_cloud_counts": (C.c_int, [_p, _p, _p]),
    "pdbeda_cloud_atom_rows": (C.c_int, [_p, _p, _p, _p, _p, _p]),
    "pdbeda_cloud_residue_rows": (C.c_int, [_p, _p, _p, _p, _p, _p]),
    "pdbeda_cloud_domain_rows": (C.c_int, [_p, _p, _p, _p, _p, _p]),
    "pdbeda_cloud_owner_states": (C.c_int, [_p, _p]),
    "pdbeda_cloud_free": (C.c_int, [_p]),
    "pdbeda_test_overlap": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _p]),
    "pdbeda_symmetry_atoms": (C.c_int, [_p, _p, _i64, _p, C.c_int32, _p, _p, _p, _p, _p, _p, _i64, C.POINTER(_i64)]),
    "pdbeda_nearest_atom": (C.c_int, [_p, _p, _i64, _p, _i64, _p, _p]),
    "pdbeda_coord_contacts": (C.c_int, [_p, _p, _i64, _p, _i64, C.c_double, _p, _p, _i64, C.POINTER(_i64)]),
    "pdbeda_crystal_contacts": (C.c_int, [_p, _p, _i64, _p, _i64, _p, C.c_int32, _p, _p, _i64, C.c_double, _p, _p, _p, _i64, C.POINTER(_i64)]),
    "pdbeda_image_coords": (C.c_int, [_p, _p, _i64, _p, C.c_int32, _p, _p, _i64, _p]),
}
EXPORTED_SYMBOLS = tuple(sorted(_SIGS))


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise PdbedaError("libpdbeda_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                                  "there is no CPU fallback" % LIB_PATH)
            handle = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(handle, name)
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context(object):
    """One device + one HIP stream (+ a cache of device arenas)."""

    def __init__(self, device=0, stream=None):
        self._lib = lib()
        h = C.c_void_p()
        rc = self._lib.pdbeda_ctx_create_on_stream(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise PdbedaError("pdbeda_ctx_create(device=%d) failed with status %d: no usable gfx950 device "
                              "(the hot path has no CPU fallback)" % (device, rc))
        self._h = h
        self.device = int(device)

    def check(self, rc, what):
        if rc != 0:
            msg = self._lib.pdbeda_last_error(self._h)
            cls = PdbedaTimeout if rc == PDBEDA_ERR_TIMEOUT else PdbedaError
            error = cls("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
            error.code = rc
            raise error

    def set_timeout(self, seconds):
        """Arm (seconds > 0: ONE deadline, now + seconds, for every wait until the next call -- re-arm it when an entry starts) or
        disarm (0) the per-entry watchdog: see pdbeda_ctx_set_timeout in include/pdbeda.h."""
        self.check(self._lib.pdbeda_ctx_set_timeout(self._h, C.c_double(float(seconds))), "pdbeda_ctx_set_timeout")

    def synchronize(self):
        self.check(self._lib.pdbeda_ctx_synchronize(self._h), "pdbeda_ctx_synchronize")

    @property
    def stream(self):
        return self._lib.pdbeda_ctx_stream(self._h)

    def profile_begin(self):
        self.check(self._lib.pdbeda_ctx_profile_begin(self._h), "pdbeda_ctx_profile_begin")

    def profile_end(self):
        """{kernel: (calls, total_ms)} measured with HIP events on this context's stream."""
        buf = C.create_string_buffer(1 << 16)
        self.check(self._lib.pdbeda_ctx_profile_end(self._h, buf, len(buf)), "pdbeda_ctx_profile_end")
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.rsplit(" ", 2)
            out[name] = (int(calls), float(ms))
        return out

    def close(self):
        """The status of pdbeda_ctx_destroy: 0, or PDBEDA_ERR_STATE when no handle was alive and the library had lost an arena
        (0 for a context that is closed already)."""
        rc = 0
        if getattr(self, "_h", None):
            rc = self._lib.pdbeda_ctx_destroy(self._h)
            self._h = None
        return rc

    # -- context-level helpers -------------------------------------------------------
    def test_overlap(self, crs, set_offsets, a_idx, b_idx):
        crs = np.ascontiguousarray(crs, dtype=np.int32).reshape(-1, 3)
        off = np.ascontiguousarray(set_offsets, dtype=np.int64)
        a = np.ascontiguousarray(a_idx, dtype=np.int32)
        b = np.ascontiguousarray(b_idx, dtype=np.int32)
        out = np.zeros(len(a), dtype=np.uint8)
        self.check(self._lib.pdbeda_test_overlap(self._h, _ptr(crs), _ptr(off), len(off) - 1, _ptr(a), _ptr(b), len(a), _ptr(out)),
                   "pdbeda_test_overlap")
        return out.astype(bool)

    def symmetry_atoms(self, xyz, rot, ortho, bbox_lo, bbox_hi):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 12)
        ortho = np.ascontiguousarray(ortho, dtype=np.float64).reshape(9)
        lo = np.ascontiguousarray(bbox_lo, dtype=np.float64)
        hi = np.ascontiguousarray(bbox_hi, dtype=np.float64)
        cap = 27 * len(rot) * len(xyz)
        idx = np.zeros(cap, dtype=np.int32)
        sym = np.zeros((cap, 4), dtype=np.int32)
        out = np.zeros((cap, 3), dtype=np.float64)
        n = C.c_int64(0)
        self.check(self._lib.pdbeda_symmetry_atoms(self._h, _ptr(xyz), len(xyz), _ptr(rot), len(rot), _ptr(ortho), _ptr(lo), _ptr(hi),
                                                   _ptr(idx), _ptr(sym), _ptr(out), cap, C.byref(n)), "pdbeda_symmetry_atoms")
        k = n.value
        return idx[:k].copy(), sym[:k].copy(), out[:k].copy()

    def nearest_atom(self, centroids, atom_xyz):
        cen = np.ascontiguousarray(centroids, dtype=np.float64).reshape(-1, 3)
        at = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        idx = np.zeros(len(cen), dtype=np.int64)
        dist = np.zeros(len(cen), dtype=np.float64)
        self.check(self._lib.pdbeda_nearest_atom(self._h, _ptr(cen), len(cen), _ptr(at), len(at), _ptr(idx), _ptr(dist)),
                   "pdbeda_nearest_atom")
        return idx, dist

    def coord_contacts(self, q_xyz, p_xyz, cutoff):
        """(index, distance) of the query points whose nearest p_xyz point is within cutoff (pdbeda_coord_contacts)."""
        q = np.ascontiguousarray(q_xyz, dtype=np.float64).reshape(-1, 3)
        p = np.ascontiguousarray(p_xyz, dtype=np.float64).reshape(-1, 3)
        idx = np.zeros(len(q), dtype=np.int64)
        dist = np.zeros(len(q), dtype=np.float64)
        n = C.c_int64(0)
        self.check(self._lib.pdbeda_coord_contacts(self._h, _ptr(q), len(q), _ptr(p), len(p), C.c_double(float(cutoff)), _ptr(idx), _ptr(dist), len(q),
                                                   C.byref(n)), "pdbeda_coord_contacts")
        return idx[:n.value].copy(), dist[:n.value].copy()

    def crystal_contacts(self, q_xyz, poly_xyz, rot, ortho, cand, cutoff):
        """(kept flag per candidate image, index, distance) of pdbeda_crystal_contacts."""
        q = np.ascontiguousarray(q_xyz, dtype=np.float64).reshape(-1, 3)
        p = np.ascontiguousarray(poly_xyz, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 12)
        ortho = np.ascontiguousarray(ortho, dtype=np.float64).reshape(9)
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1, 4)
        kept = np.zeros(len(cand), dtype=np.uint8)
        idx = np.zeros(len(q), dtype=np.int64)
        dist = np.zeros(len(q), dtype=np.float64)
        n = C.c_int64(0)
        self.check(self._lib.pdbeda_crystal_contacts(self._h, _ptr(q), len(q), _ptr(p), len(p), _ptr(rot), len(rot), _ptr(ortho), _ptr(cand), len(cand),
                                                     C.c_double(float(cutoff)), _ptr(kept), _ptr(idx), _ptr(dist), len(q), C.byref(n)),
                   "pdbeda_crystal_contacts")
        return kept.astype(bool), idx[:n.value].copy(), dist[:n.value].copy()

    def image_coords(self, poly_xyz, rot, ortho, cand):
        """The points of the listed images in (image, point) order, as an (n_cand * n_poly, 3) array (pdbeda_image_coords)."""
        p = np.ascontiguousarray(poly_xyz, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 12)
        ortho = np.ascontiguousarray(ortho, dtype=np.float64).reshape(9)
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((len(cand) * len(p), 3), dtype=np.float64)
        self.check(self._lib.pdbeda_image_coords(self._h, _ptr(p), len(p), _ptr(rot), len(rot), _ptr(ortho), _ptr(cand), len(cand), _ptr(out)),
                   "pdbeda_image_coords")
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}
_default_lock = threading.Lock()


def device_local_cpus(device=0):
    """Host cores on the NUMA node of GPU ``device`` (sysfs ``local_cpulist`` of its PCI function), or None when the
    platform does not say (no sysfs, a single node, a container that hides it)."""
    buf = C.create_string_buffer(64)
    if lib().pdbeda_device_pci_address(int(device), buf, 64) != 0:
        return None
    address = buf.value.decode().strip().lower()
    try:
        with open("/sys/bus/pci/devices/%s/local_cpulist" % address) as fh:
            text = fh.read().strip()
    except OSError:
        return None
    cpus = set()
    for part in text.split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus or None


def pin_to_device(device=0):
    """Restrict the calling thread (and the threads and processes it starts afterwards) to the cores of the GPU's NUMA node:
    file reads, parsing and the pageable side of every upload then stay on the socket the GPU hangs off.  Returns the number
    of cores kept, or 0 when nothing was changed."""
    if not hasattr(os, "sched_setaffinity"):
        return 0
    local = device_local_cpus(device)
    if not local:
        return 0
    keep = local & os.sched_getaffinity(0)
    if not keep or keep == os.sched_getaffinity(0):
        return 0
    os.sched_setaffinity(0, keep)
    return len(keep)


def default_context(device=None):
    """Per-thread default context (device from PDBEDA_DEVICE / LOCAL_RANK, else 0)."""
    if device is None:
        device = int(os.environ.get("PDBEDA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    key = (threading.get_ident(), device)
    with _default_lock:
        ctx = _default_ctx.get(key)
        if ctx is None:
            ctx = Context(device)
            _default_ctx[key] = ctx
    return ctx


class BlobList(object):
    """Result of a labelling call; statistics and voxel membership are fetched on demand."""

    def __init__(self, ctx, handle, keepalive=None):
        self._ctx = ctx
        self._h = handle
        self._keep = keepalive
        self._stats = None
        self._vox = None

    def __len__(self):
        n = self._ctx._lib.pdbeda_bloblist_count(self._h)
        if n < 0:
            self._ctx.check(int(n), "pdbeda_bloblist_count")
        return int(n)

    def stats(self):
        if self._stats is None:
            n = len(self)
            st = {"n": np.zeros(n, np.int64), "totalDensity": np.zeros(n, np.float64), "centroid": np.zeros((n, 3), np.float64),
                  "coordCenter": np.zeros((n, 3), np.float64), "volume": np.zeros(n, np.float64), "firstKey": np.zeros(n, np.int64),
                  "group": np.zeros(n, np.int32)}
            self._ctx.check(self._ctx._lib.pdbeda_bloblist_stats(self._h, _ptr(st["n"]), _ptr(st["totalDensity"]), _ptr(st["centroid"]),
                                                                 _ptr(st["coordCenter"]), _ptr(st["volume"]), _ptr(st["firstKey"]),
                                                                 _ptr(st["group"])), "pdbeda_bloblist_stats")
            self._stats = st
        return self._stats

    def voxels(self):
        """(crs[N,3] int32 grouped by blob, offsets[count+1])."""
        if self._vox is None:
            nv = self._ctx._lib.pdbeda_bloblist_num_voxels(self._h)
            if nv < 0:
                self._ctx.check(int(nv), "pdbeda_bloblist_num_voxels")
            crs = np.zeros((int(nv), 3), dtype=np.int32)
            off = np.zeros(len(self) + 1, dtype=np.int64)
            self._ctx.check(self._ctx._lib.pdbeda_bloblist_voxels(self._h, _ptr(crs), _ptr(off)), "pdbeda_bloblist_voxels")
            self._vox = (crs, off)
        return self._vox

    def voxels_of(self, i):
        crs, off = self.voxels()
        return crs[off[i]:off[i + 1]]

    def moments(self):
        """pdbeda_bloblist_moments: per blob, in list order, ``boxLo`` / ``boxHi`` / ``extremeCrs`` (n x 3 int32), ``extreme`` (float32),
        the exact offset sums ``s1`` (n x 3) / ``s2`` (n x 6, int64) and the |density|-weighted ``sw`` (n), ``sw1`` (n x 3), ``sw2`` (n x 6)."""
        n = len(self)
        out = {"boxLo": np.zeros((n, 3), np.int32), "boxHi": np.zeros((n, 3), np.int32), "extremeCrs": np.zeros((n, 3), np.int32),
               "extreme": np.zeros(n, np.float32), "s1": np.zeros((n, 3), np.int64), "s2": np.zeros((n, 6), np.int64),
               "sw": np.zeros(n, np.float64), "sw1": np.zeros((n, 3), np.float64), "sw2": np.zeros((n, 6), np.float64)}
        self._ctx.check(self._ctx._lib.pdbeda_bloblist_moments(self._h, *[_ptr(out[k]) for k in ("boxLo", "boxHi", "extremeCrs", "extreme", "s1", "s2", "sw", "sw1", "sw2")]),
                        "pdbeda_bloblist_moments")
        return out

    def nearest(self, other, offsets):
        """pdbeda_bloblist_nearest: per blob of this list, in list order, ``index`` (the first entry of the ordered ``offsets`` table, n x 3 int32,
        that leads from a voxel of the blob into a blob of ``other``; -1 without one), ``partner`` (that blob's index in ``other``, or -1) and the two
        voxels ``voxel`` / ``partnerVoxel`` (n x 3 int32, zeros without a partner)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        n = len(self)
        out = {"index": np.zeros(n, np.int32), "partner": np.zeros(n, np.int32), "voxel": np.zeros((n, 3), np.int32), "partnerVoxel": np.zeros((n, 3), np.int32)}
        self._ctx.check(self._ctx._lib.pdbeda_bloblist_nearest(self._h, other._h if other is not None else None, _ptr(offsets) if len(offsets) else None, len(offsets),
                                                               _ptr(out["index"]), _ptr(out["partner"]), _ptr(out["voxel"]), _ptr(out["partnerVoxel"])),
                        "pdbeda_bloblist_nearest")
        return out

    def labels(self, shape):
        out = np.zeros(shape, dtype=np.int32)
        self._ctx.check(self._ctx._lib.pdbeda_bloblist_labels(self._h, _ptr(out)), "pdbeda_bloblist_labels")
        return out

    def counters(self):
        out = np.zeros(8, dtype=np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_bloblist_counters(self._h, _ptr(out)), "pdbeda_bloblist_counters")
        return {"run_ids": int(out[0]), "component_ids": int(out[1]), "blobs": int(out[3]), "unit_tiles_runs": int(out[4]), "wide_tiles": int(out[5]), "unit_tiles_comps": int(out[6]),
                "reruns": int(out[2]), "arena_bytes": int(out[7])}

    def free(self):
        if self._h is not None and self._ctx._h:
            self._ctx._lib.pdbeda_bloblist_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PeakList(object):
    """Result of a peak search (pdbeda_map_peaks): the columns are fetched on demand, in list order."""

    def __init__(self, ctx, handle, keepalive=None):
        self._ctx = ctx
        self._h = handle
        self._keep = keepalive             # the map and the blob list(s) the job reads
        self._rows = None

    def __len__(self):
        n = self._ctx._lib.pdbeda_peaklist_count(self._h)
        if n < 0:
            self._ctx.check(int(n), "pdbeda_peaklist_count")
        return int(n)

    def rows(self):
        """{"crs" n x 3 int32, "height" float32, "xyz" n x 3, "refinedHeight", "blob" int32, "onBorder" bool}."""
        if self._rows is None:
            n = len(self)
            st = {"crs": np.zeros((n, 3), np.int32), "height": np.zeros(n, np.float32), "xyz": np.zeros((n, 3), np.float64),
                  "refinedHeight": np.zeros(n, np.float64), "blob": np.zeros(n, np.int32), "onBorder": np.zeros(n, np.uint8)}
            self._ctx.check(self._ctx._lib.pdbeda_peaklist_rows(self._h, _ptr(st["crs"]), _ptr(st["height"]), _ptr(st["xyz"]), _ptr(st["refinedHeight"]),
                                                                _ptr(st["blob"]), _ptr(st["onBorder"])), "pdbeda_peaklist_rows")
            st["onBorder"] = st["onBorder"].astype(bool)
            self._rows = st
        return self._rows

    def counters(self):
        out = np.zeros(4, dtype=np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_peaklist_counters(self._h, _ptr(out)), "pdbeda_peaklist_counters")
        return {"tested": int(out[0]), "peaks": int(out[1]), "reruns": int(out[2]), "arena_bytes": int(out[3])}

    def basins(self, volume=False):
        """pdbeda_peaklist_basins: per peak, in list order, ``n`` (int64), ``sum``, ``s1`` (n x 3 int64), ``sw1`` (n x 3), ``saddle`` (float32),
        ``neighbour`` (int32); ``counters`` {"significant", "orphans", "rounds", "arena_bytes"}; with ``volume`` also ``basin``, the int32
        volume over the box's voxels ([s][r][c] of the box, c fastest)."""
        n = len(self)
        out = {"n": np.zeros(n, np.int64), "sum": np.zeros(n, np.float64), "s1": np.zeros((n, 3), np.int64), "sw1": np.zeros((n, 3), np.float64),
               "saddle": np.zeros(n, np.float32), "neighbour": np.zeros(n, np.int32)}
        vol = None
        if volume:
            vol = np.zeros(self._keep[0].unique_shape, np.int32)
        ctr = np.zeros(4, np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_peaklist_basins(self._h, *([_ptr(out[k]) for k in ("n", "sum", "s1", "sw1", "saddle", "neighbour")] + [_ptr(vol), _ptr(ctr)])),
                        "pdbeda_peaklist_basins")
        out["counters"] = {"significant": int(ctr[0]), "orphans": int(ctr[1]), "rounds": int(ctr[2]), "arena_bytes": int(ctr[3])}
        if volume:
            out["basin"] = vol
        return out

    def free(self):
        if self._h is not None and self._ctx._h:
            self._ctx._lib.pdbeda_peaklist_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def radix_select(digit, bits, ranks):
    """The host side of the radix select of ``DeviceMap.abs_order_statistics``: the ``bits``-bit keys (Python ints) at the 0-based
    ``ranks`` of the ascending order, found 16 bits a pass from the most significant digit down.  ``digit(shift, prefix, mask)`` returns
    the 65536-bin histogram (int64) of bits [shift, shift + 16) of the keys that agree with ``prefix`` on ``mask``."""
    out = []
    for rank in ranks:
        prefix, mask, remaining = 0, 0, int(rank)
        for shift in range(bits - 16, -1, -16):
            cs = np.cumsum(digit(shift, prefix, mask))
            d = int(np.searchsorted(cs, remaining, side="right"))
            remaining -= int(cs[d - 1]) if d else 0
            prefix |= d << shift
            mask |= 0xffff << shift
        out.append(prefix)
    return out


FILTER_MAX_RADIUS = 64           # PDBEDA_FILTER_MAX_RADIUS
FILTER_RENORMALIZE = 1           # PDBEDA_FILTER_RENORMALIZE
SPREAD_MAX_OFFSETS = 16384       # PDBEDA_SPREAD_MAX_OFFSETS
SPREAD_MAX_REACH = 32            # PDBEDA_SPREAD_MAX_REACH
SPREAD_BELOW = 1                 # PDBEDA_SPREAD_BELOW
MOMENTS_UNIQUE_BOX = 1           # PDBEDA_MOMENTS_UNIQUE_BOX
POSE_ALLOW_OUTSIDE, POSE_GLOBAL_ONLY = 1, 2      # PDBEDA_POSE_ALLOW_OUTSIDE, PDBEDA_POSE_GLOBAL_ONLY
POSE_MAX_ATOMS, POSE_MAX_ROTATIONS, POSE_MAX_TOP = 256, 1 << 20, 64
LOCAL_STATS_OUTPUTS = ("mean_a", "std_a", "z_a", "mean_b", "std_b", "cc")      # the output pointers of pdbeda_map_local_stats, in order


def _filter_taps(*taps):
    """The taps of the three axes as float64 arrays of odd length (a radius the library refuses is passed on as it is)."""
    out = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in taps]
    if any(len(t) % 2 == 0 for t in out):
        raise ValueError("filter taps have an odd length, 2 * radius + 1")
    return out


RESAMPLE_MAX_OPS = 192           # PDBEDA_RESAMPLE_MAX_OPS
RESAMPLE_MEAN = 1                # PDBEDA_RESAMPLE_MEAN
RESAMPLE_COUNTERS = ("covered", "uncovered", "stagedPairs", "directPairs")      # the counters of pdbeda_map_resample, in order


FFT_MAX_AXIS = 1024              # PDBEDA_FFT_MAX_AXIS
SPECTRUM_MAX_TABLE = 4096        # PDBEDA_SPECTRUM_MAX_TABLE
SPECTRUM_MAX_SHELLS = 256        # PDBEDA_SPECTRUM_MAX_SHELLS


class DeviceSpectrum(object):
    """The Hermitian half spectrum of a map, resident in HBM (pdbeda_map_fft): complex fp64 [ns][nr][nc / 2 + 1], numpy's rfftn."""

    def __init__(self, ctx, handle):
        self._ctx, self._h = ctx, handle
        ncrs = np.zeros(3, dtype=np.int32)
        ctx.check(ctx._lib.pdbeda_spectrum_shape(handle, _ptr(ncrs)), "pdbeda_spectrum_shape")
        self.ncrs = tuple(int(v) for v in ncrs)
        self.shape = (self.ncrs[2], self.ncrs[1], self.ncrs[0] // 2 + 1)

    def download(self):
        """The coefficients as a complex128 array [ns][nr][nc / 2 + 1]."""
        out = np.empty(self.shape, dtype=np.complex128)
        self._ctx.check(self._ctx._lib.pdbeda_spectrum_download(self._h, _ptr(out)), "pdbeda_spectrum_download")
        return out

    def values(self, idx):
        """pdbeda_spectrum_values: the coefficients at the (n, 3) integer indices ``idx`` (crs order; any integer, either half)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(len(idx), dtype=np.complex128)
        self._ctx.check(self._ctx._lib.pdbeda_spectrum_values(self._h, _ptr(idx) if len(idx) else None, len(idx), _ptr(out) if len(idx) else None), "pdbeda_spectrum_values")
        return out

    def scale(self, metric, table, s2_max, beyond=0.0):
        """pdbeda_spectrum_scale: every coefficient times the table's g(s^2), IN PLACE."""
        metric = np.ascontiguousarray(metric, dtype=np.float64).reshape(6)
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        self._ctx.check(self._ctx._lib.pdbeda_spectrum_scale(self._h, _ptr(metric), _ptr(table), len(table), C.c_double(float(s2_max)), C.c_double(float(beyond))),
                        "pdbeda_spectrum_scale")

    def shells(self, other, metric, edges):
        """pdbeda_spectrum_shells: (count int64 [n], sums float64 [n][4]) over the shells between the ``edges`` of s^2."""
        metric = np.ascontiguousarray(metric, dtype=np.float64).reshape(6)
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        n = len(edges) - 1
        count, sums = np.zeros(max(n, 0), dtype=np.int64), np.zeros((max(n, 0), 4), dtype=np.float64)
        self._ctx.check(self._ctx._lib.pdbeda_spectrum_shells(self._h, other._h if other is not None else None, _ptr(metric), _ptr(edges), n, _ptr(count), _ptr(sums)),
                        "pdbeda_spectrum_shells")
        return count, sums

    def inverse(self, like):
        """pdbeda_spectrum_inverse: a new resident map on the geometry of the DeviceMap ``like``."""
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_spectrum_inverse(self._h, like._h, C.byref(h)), "pdbeda_spectrum_inverse")
        return DeviceMap._made(like, h)

    def free(self):
        if getattr(self, "_h", None) is not None and self._ctx._h:
            self._ctx._lib.pdbeda_spectrum_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceMap(object):
    """A density grid resident in HBM + its unit-cell basis."""

    def __init__(self, ctx, density, geometry, device_ptr=None):
        self._ctx = ctx
        self._geom = geometry
        h = C.c_void_p()
        if device_ptr is not None:
            rc = ctx._lib.pdbeda_map_from_device(ctx._h, C.c_void_p(device_ptr), C.byref(geometry), C.byref(h))
            self._keep = density
        else:
            grid = np.ascontiguousarray(density, dtype=np.float32)
            assert grid.size == geometry.ncrs[0] * geometry.ncrs[1] * geometry.ncrs[2], "grid size does not match header ncrs"
            mean, std = C.c_double(), C.c_double()      # (with the map's mean / std from the same wait: every caller asks for them next)
            rc = ctx._lib.pdbeda_map_upload_stats(ctx._h, _ptr(grid), C.byref(geometry), C.byref(h), C.byref(mean), C.byref(std))
            if rc == 0:
                self._file_stats = (mean.value, std.value)
            self._keep = None
        ctx.check(rc, "pdbeda_map_upload")
        self._h = h
        self.unique_shape = tuple(min(geometry.ncrs[k], geometry.xyz_interval[geometry.map2crs[k]]) for k in (2, 1, 0))

    def invalidate(self):
        """The caller rewrote a borrowed device buffer in place: drop what the library cached about its contents."""
        self._ctx.check(self._ctx._lib.pdbeda_map_invalidate(self._h), "pdbeda_map_invalidate")
        self.__dict__.pop("_file_stats", None)

    @classmethod
    def from_file(cls, ctx, path, offset, byteswap, geometry):
        """The float32 grid stored at byte ``offset`` of ``path`` straight into HBM through the process's upload engine (three reader
        threads with pinned chunks and copy streams of their own: file reads and PCIe copies overlap; no host copy of the map is kept)."""
        self = cls.__new__(cls)
        self._ctx, self._geom, self._keep = ctx, geometry, None
        h = C.c_void_p()
        mean, std = C.c_double(), C.c_double()
        try:
            # (with the map's mean / std from the same wait: every caller asks for them next)
            ctx.check(ctx._lib.pdbeda_map_upload_file_stats(ctx._h, os.fsencode(path), int(offset), 1 if byteswap else 0, C.byref(geometry), C.byref(h),
                                                            C.byref(mean), C.byref(std)), "pdbeda_map_upload_file")
            self._file_stats = (mean.value, std.value)
        except PdbedaError as error:
            if getattr(error, "code", 0) == PDBEDA_ERR_ARGUMENT:       # the FILE is at fault (unreadable, truncated): an entry-level condition
                raise OSError(str(error))
            raise
        self._h = h
        self.unique_shape = tuple(min(geometry.ncrs[k], geometry.xyz_interval[geometry.map2crs[k]]) for k in (2, 1, 0))
        return self

    @classmethod
    def combine(cls, a, b, alpha):
        """A new resident map: float32(double(a) + alpha * double(b)) per voxel, on the geometry of ``a`` (device side)."""
        self = cls.__new__(cls)
        self._ctx, self._geom, self._keep, self.unique_shape = a._ctx, a._geom, None, a.unique_shape
        h = C.c_void_p()
        a._ctx.check(a._ctx._lib.pdbeda_map_combine(a._h, b._h, C.c_double(alpha), C.byref(h)), "pdbeda_map_combine")
        self._h = h
        return self

    @classmethod
    def model_density(cls, like, xyz, amp, expo, radii):
        """pdbeda_model_density: a new resident map on the geometry of ``like`` -- the density of the Gaussian atoms ``xyz`` (n x 3), each
        ``amp[a][j] * exp(-expo[a][j] * d^2)`` summed over its terms and cut off at ``radii[a]``; ``amp`` / ``expo`` are (n,) or
        (n, n_terms).  The map carries ``model_counters``: {"shift", "maxStaged", "multiRunTiles"}."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        na = len(xyz)
        amp = np.ascontiguousarray(amp, dtype=np.float64).reshape(na, -1) if na else np.zeros((0, 1))      # (no atom: one term of nothing)
        expo = np.ascontiguousarray(expo, dtype=np.float64).reshape(na, -1) if na else np.zeros((0, 1))
        radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        if amp.shape != expo.shape or len(radii) != na:
            raise ValueError("amp and expo must have one shape, (n_atoms, n_terms), and radii one value per atom")
        self = cls.__new__(cls)
        self._ctx, self._geom, self._keep, self.unique_shape = like._ctx, like._geom, None, like.unique_shape
        h = C.c_void_p()
        ctr = np.zeros(3, dtype=np.int64)
        like._ctx.check(like._ctx._lib.pdbeda_model_density(like._h, _ptr(xyz) if na else None, na, int(amp.shape[1]), _ptr(amp) if na else None, _ptr(expo) if na else None,
                                                            _ptr(radii) if na else None, C.byref(h), _ptr(ctr)), "pdbeda_model_density")
        self._h = h
        self.model_counters = {"shift": int(ctr[0]), "maxStaged": int(ctr[1]), "multiRunTiles": int(ctr[2])}
        return self

    def pair_moments(self, other, floor=None):
        """pdbeda_map_pair_moments: (n, [Sa, Sb, Saa, Sbb, Sab]) over the voxels of the unique box where this map (a) and ``other`` (b) are
        finite and b > float32(floor) (strict; None: every finite pair)."""
        n = C.c_int64(0)
        sums = np.zeros(5, dtype=np.float64)
        self._ctx.check(self._ctx._lib.pdbeda_map_pair_moments(self._h, other._h, C.c_float(-np.inf if floor is None else floor), C.byref(n), _ptr(sums)),
                        "pdbeda_map_pair_moments")
        return int(n.value), sums

    def atom_moments(self, xyz, expo, radii, unique_box=False):
        """pdbeda_atom_moments: the adjoint of ``model_density`` with this map as the weight -- per atom and term the sums M0, Mx, My, Mz, M2 of
        w e, w e dx, w e dy, w e dz, w e d^2 (e = exp(-expo d^2)) over the voxels within ``radii[a]``, over all stored voxels or, with
        ``unique_box``, over the non-repeating box.  ``expo`` is (n,) or (n, n_terms).  A dict: ``moments`` (n, n_terms, 5), ``nVoxels`` (n,)
        int32 and ``counters`` {"shift", "maxBoxVoxels", "clippedAtoms"}."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        na = len(xyz)
        expo = np.ascontiguousarray(expo, dtype=np.float64).reshape(na, -1) if na else np.zeros((0, 1))
        radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        if len(radii) != na:
            raise ValueError("radii must have one value per atom")
        moments = np.zeros((na, expo.shape[1], 5), dtype=np.float64)
        n_voxels = np.zeros(na, dtype=np.int32)
        ctr = np.zeros(3, dtype=np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_atom_moments(self._h, _ptr(xyz) if na else None, na, int(expo.shape[1]), _ptr(expo) if na else None, _ptr(radii) if na else None,
                                                           MOMENTS_UNIQUE_BOX if unique_box else 0, _ptr(moments) if na else None, _ptr(n_voxels) if na else None, _ptr(ctr)),
                        "pdbeda_atom_moments")
        return {"moments": moments, "nVoxels": n_voxels, "counters": {"shift": int(ctr[0]), "maxBoxVoxels": int(ctr[1]), "clippedAtoms": int(ctr[2])}}

    def pose_scores(self, frag_xyz, frag_w, rot, centres, top_k=1, floor=-np.inf, max_low=None, allow_outside=False, full=False, global_only=False):
        """pdbeda_pose_scores: the rigid fragment ``frag_xyz`` (n_frag x 3, relative to its pivot; weights ``frag_w``) under every rotation of
        ``rot`` (n_rot x 3 x 3) at every centre of ``centres`` (n x 3) on this map.  A pose scores sum_a w_a * (the trilinear density at its atom
        a); it is rejected when more than ``max_low`` atoms (None: never) read less than ``floor``, when its score is NaN, or -- unless
        ``allow_outside`` -- when an atom reads a voxel that is not stored.  A dict: ``bestRot`` / ``bestScore`` / ``bestLow`` (n, top_k: the kept
        poses of a centre, best first, -1 / +0.0 / 0 beyond them), ``nKept`` (n,), with ``full`` the tables ``scores`` / ``low`` / ``kept``
        (n, n_rot), and ``counters`` {"globalCentres", "maxStagedBox", "rejected"}.  ``global_only``: no box is staged in LDS (an A/B switch)."""
        frag_xyz = np.ascontiguousarray(frag_xyz, dtype=np.float64).reshape(-1, 3)
        frag_w = np.ascontiguousarray(frag_w, dtype=np.float64).reshape(-1)
        rot = np.ascontiguousarray(rot, dtype=np.float64).reshape(-1, 9)
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
        if len(frag_w) != len(frag_xyz):
            raise ValueError("frag_w must have one weight per fragment atom")
        n, nr, k = len(centres), len(rot), int(top_k)
        rows = max(k, 0)
        best_rot, best_score, best_low = np.full((n, rows), -1, dtype=np.int32), np.zeros((n, rows), dtype=np.float64), np.zeros((n, rows), dtype=np.int32)
        n_kept = np.zeros(n, dtype=np.int32)
        score = np.zeros((n, nr), dtype=np.float64) if full else None
        low = np.zeros((n, nr), dtype=np.int32) if full else None
        kept = np.zeros((n, nr), dtype=np.uint8) if full else None
        ctr = np.zeros(3, dtype=np.int64)
        flags = (POSE_ALLOW_OUTSIDE if allow_outside else 0) | (POSE_GLOBAL_ONLY if global_only else 0)
        self._ctx.check(self._ctx._lib.pdbeda_pose_scores(self._h, _ptr(frag_xyz), _ptr(frag_w), len(frag_xyz), _ptr(rot), nr, _ptr(centres) if n else None, n,
                                                          C.c_float(floor), 2 ** 31 - 1 if max_low is None else int(max_low), k, flags,
                                                          _ptr(best_rot), _ptr(best_score), _ptr(best_low), _ptr(n_kept), _ptr(score), _ptr(low), _ptr(kept), _ptr(ctr)),
                        "pdbeda_pose_scores")
        out = {"bestRot": best_rot, "bestScore": best_score, "bestLow": best_low, "nKept": n_kept,
               "counters": {"globalCentres": int(ctr[0]), "maxStagedBox": int(ctr[1]), "rejected": int(ctr[2])}}
        if full:
            out.update(scores=score, low=low, kept=kept.astype(bool))
        return out

    @classmethod
    def _made(cls, like, h):
        """A map the library made on the geometry of ``like`` (handle ``h``)."""
        self = cls.__new__(cls)
        self._ctx, self._geom, self._keep, self.unique_shape = like._ctx, like._geom, None, like.unique_shape
        self._h = h
        return self

    def filter(self, taps_c, taps_r, taps_s, renormalize=False):
        """pdbeda_map_filter: a new resident map, this one filtered along c, r and s with the given taps (odd lengths 2 R + 1, correlation
        form, the map's wrap rule at the faces); ``renormalize`` divides by the weight of the taps that met a voxel."""
        taps = _filter_taps(taps_c, taps_r, taps_s)
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_map_filter(self._h, _ptr(taps[0]), len(taps[0]) // 2, _ptr(taps[1]), len(taps[1]) // 2, _ptr(taps[2]), len(taps[2]) // 2,
                                                         FILTER_RENORMALIZE if renormalize else 0, C.byref(h)), "pdbeda_map_filter")
        return type(self)._made(self, h)

    def spread(self, offsets, values, threshold=0.5, below=False, base=None, counters=False):
        """pdbeda_map_spread: a new resident map -- per stored voxel ``values[t]`` (times ``base``'s voxel, rounded once), t the first entry of the
        ordered ``offsets`` table (n x 3 int32: dc, dr, ds) that leads to a seed (a voxel > ``threshold``, or < it with ``below``) under the map's
        wrap rule, and n without one: ``values`` has n + 1 float32 entries.  With ``counters`` the result is (map, {"seeds", "reached", "rows"})."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, 3)
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if len(values) != len(offsets) + 1:
            raise ValueError("values must have one entry per offset and a last one for no seed in reach")
        h = C.c_void_p()
        ctr = np.zeros(3, dtype=np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_map_spread(self._h, C.c_float(threshold), SPREAD_BELOW if below else 0, _ptr(offsets) if len(offsets) else None, len(offsets),
                                                         _ptr(values), base._h if base is not None else None, C.byref(h), _ptr(ctr)), "pdbeda_map_spread")
        made = type(self)._made(self, h)
        return (made, {"seeds": int(ctr[0]), "reached": int(ctr[1]), "rows": int(ctr[2])}) if counters else made

    def local_stats(self, other, taps_c, taps_r, taps_s, std_floor=0.0, want=None):
        """pdbeda_map_local_stats: a dict of new resident maps out of ``mean_a``, ``std_a``, ``z_a`` and, with ``other``, ``mean_b``, ``std_b``,
        ``cc`` -- all that apply, or the names in ``want``."""
        names = LOCAL_STATS_OUTPUTS if other is not None else LOCAL_STATS_OUTPUTS[:3]
        want = names if want is None else tuple(want)
        if any(name not in LOCAL_STATS_OUTPUTS for name in want):
            raise ValueError("local_stats outputs are %s" % ", ".join(LOCAL_STATS_OUTPUTS))
        taps = _filter_taps(taps_c, taps_r, taps_s)
        handles = dict((name, C.c_void_p()) for name in want)
        refs = [C.byref(handles[name]) if name in handles else None for name in LOCAL_STATS_OUTPUTS]
        self._ctx.check(self._ctx._lib.pdbeda_map_local_stats(self._h, other._h if other is not None else None, _ptr(taps[0]), len(taps[0]) // 2, _ptr(taps[1]), len(taps[1]) // 2,
                                                              _ptr(taps[2]), len(taps[2]) // 2, C.c_double(float(std_floor)), *refs), "pdbeda_map_local_stats")
        return dict((name, type(self)._made(self, handles[name])) for name in want)

    def resample(self, geometry, ops, order=1, mean=False, fill=0.0, base=None, alpha=1.0, coverage=False):
        """pdbeda_map_resample: a new resident map on ``geometry`` -- every voxel of it pulled back into this map through the operators
        ``ops`` (n x 12 rows of [R | t], destination to source coordinates) and read at ``order`` 0, 1 or 3: the first valid operator, or
        with ``mean`` the average over the valid ones; ``fill`` where none is; with ``base`` (on ``geometry``) base + alpha * value.
        Returns (map, coverage map or None); the map carries ``resample_counters``.  ``fill`` is passed as a float32 with its bits kept."""
        ops = np.ascontiguousarray(ops, dtype=np.float64).reshape(-1, 12)
        fill32 = C.c_float.from_buffer_copy(np.asarray(fill, dtype=np.float32).tobytes())
        h, hc = C.c_void_p(), C.c_void_p()
        ctr = np.zeros(4, dtype=np.int64)
        self._ctx.check(self._ctx._lib.pdbeda_map_resample(self._h, C.byref(geometry), _ptr(ops) if len(ops) else None, len(ops), int(order), RESAMPLE_MEAN if mean else 0, fill32,
                                                           base._h if base is not None else None, C.c_double(float(alpha)), C.byref(h), C.byref(hc) if coverage else None, _ptr(ctr)),
                        "pdbeda_map_resample")
        made = []
        for handle in (h, hc) if coverage else (h,):
            m = type(self).__new__(type(self))
            m._ctx, m._geom, m._keep, m._h = self._ctx, geometry, None, handle
            m.unique_shape = tuple(min(geometry.ncrs[k], geometry.xyz_interval[geometry.map2crs[k]]) for k in (2, 1, 0))
            made.append(m)
        made[0].resample_counters = dict(zip(RESAMPLE_COUNTERS, (int(v) for v in ctr)))
        return made[0], (made[1] if coverage else None)

    def abs_order_statistics(self, other, alpha, cut_a, cut_b, which, ranks=None):
        """Exact order statistics of |a| (which = 0) or |a + alpha * other| (which = 1) over the voxels of the unique box with
        |a| < cut_a and |a + alpha other| < cut_b: a radix select, 16 bits per device pass.  ranks=None -> the number of
        selected voxels; else the values at those 0-based ranks (ascending), as float64."""
        hist = np.zeros(65536, dtype=np.uint32)
        oh = other._h if other is not None else None

        def digit(shift, prefix, mask):
            self._ctx.check(self._ctx._lib.pdbeda_abs_select_hist(self._h, oh, C.c_double(alpha), C.c_double(cut_a), C.c_double(cut_b), which, shift,
                                                                  C.c_ulonglong(prefix), C.c_ulonglong(mask), _ptr(hist)), "pdbeda_abs_select_hist")
            return hist.astype(np.int64)
        bits = 64 if which else 32
        if ranks is None:
            return int(digit(bits - 16, 0, 0).sum())
        keys = radix_select(digit, bits, ranks)
        return [np.array([k], dtype=np.uint64).view(np.float64)[0] if which else float(np.array([k], dtype=np.uint32).view(np.float32)[0]) for k in keys]

    def fft(self):
        """pdbeda_map_fft: the Hermitian half spectrum of this map as a DeviceSpectrum."""
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_map_fft(self._h, C.byref(h)), "pdbeda_map_fft")
        return DeviceSpectrum(self._ctx, h)

    def download(self):
        """The float32 grid [ns][nr][nc] copied back to the host."""
        g = self._geom
        out = np.empty((g.ncrs[2], g.ncrs[1], g.ncrs[0]), dtype=np.float32)
        self._ctx.check(self._ctx._lib.pdbeda_map_download(self._h, _ptr(out)), "pdbeda_map_download")
        return out

    # -- reductions ------------------------------------------------------------------
    def stats(self):
        known = self.__dict__.get("_file_stats")           # (a map uploaded from a file brought them along)
        if known is not None:
            return known
        mean, std = C.c_double(), C.c_double()
        self._ctx.check(self._ctx._lib.pdbeda_map_stats(self._h, C.byref(mean), C.byref(std)), "pdbeda_map_stats")
        return mean.value, std.value

    def sum_of_abs(self, cutoff):
        out = C.c_double()
        self._ctx.check(self._ctx._lib.pdbeda_sum_of_abs(self._h, C.c_float(cutoff), C.byref(out)), "pdbeda_sum_of_abs")
        return out.value

    # -- points ----------------------------------------------------------------------
    def point_density(self, crs):
        crs = np.ascontiguousarray(crs, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(len(crs), dtype=np.float64)
        self._ctx.check(self._ctx._lib.pdbeda_point_density(self._h, _ptr(crs), len(crs), _ptr(out)), "pdbeda_point_density")
        return out

    def valid_crs(self, crs):
        crs = np.ascontiguousarray(crs, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(len(crs), dtype=np.uint8)
        self._ctx.check(self._ctx._lib.pdbeda_valid_crs(self._h, _ptr(crs), len(crs), _ptr(out)), "pdbeda_valid_crs")
        return out.astype(bool)

    def crs2xyz(self, crs):
        crs = np.ascontiguousarray(crs, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(crs), 3), dtype=np.float64)
        self._ctx.check(self._ctx._lib.pdbeda_crs2xyz(self._h, _ptr(crs), len(crs), _ptr(out)), "pdbeda_crs2xyz")
        return out

    def xyz2crs(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(xyz), 3), dtype=np.int32)
        self._ctx.check(self._ctx._lib.pdbeda_xyz2crs(self._h, _ptr(xyz), len(xyz), _ptr(out)), "pdbeda_xyz2crs")
        return out

    # -- labelling -------------------------------------------------------------------
    def full_blobs(self, cutoff, labels=False):
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_full_blobs(self._h, C.c_float(cutoff), PDBEDA_FLAG_LABELS if labels else 0, C.byref(h)),
                        "pdbeda_full_blobs")
        return BlobList(self._ctx, h, self)

    def full_blobs_pm(self, cutoff_pos, cutoff_neg, labels=False):
        g, r = C.c_void_p(), C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_full_blobs_pm(self._h, C.c_float(cutoff_pos), C.c_float(cutoff_neg),
                                                            PDBEDA_FLAG_LABELS if labels else 0, C.byref(g), C.byref(r)),
                        "pdbeda_full_blobs_pm")
        return BlobList(self._ctx, g, self), BlobList(self._ctx, r, self)

    def peaks(self, cutoff, blobs=None):
        """Local extrema beyond ``cutoff`` (pdbeda_map_peaks); blobs: the BlobList of ``full_blobs(cutoff)`` or None."""
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_map_peaks(self._h, C.c_float(cutoff), blobs._h if blobs is not None else None, C.byref(h)),
                        "pdbeda_map_peaks")
        return PeakList(self._ctx, h, (self, blobs))

    def peaks_pm(self, cutoff_pos, cutoff_neg, green=None, red=None):
        p, n = C.c_void_p(), C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_map_peaks_pm(self._h, C.c_float(cutoff_pos), C.c_float(cutoff_neg), green._h if green is not None else None,
                                                           red._h if red is not None else None, C.byref(p), C.byref(n)), "pdbeda_map_peaks_pm")
        return PeakList(self._ctx, p, (self, green, red)), PeakList(self._ctx, n, (self, green, red))

    def sphere_blobs(self, xyz, radii, group_offsets, cutoff):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        radii = np.ascontiguousarray(radii, dtype=np.float32)
        off = np.ascontiguousarray(group_offsets, dtype=np.int64)
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_sphere_blobs(self._h, _ptr(xyz), _ptr(radii), len(xyz), _ptr(off), len(off) - 1,
                                                           C.c_float(cutoff), C.byref(h)), "pdbeda_sphere_blobs")
        return BlobList(self._ctx, h, self)

    def list_blobs(self, crs, group_offsets=None):
        crs = np.ascontiguousarray(crs, dtype=np.int32).reshape(-1, 3)
        off = np.array([0, len(crs)], dtype=np.int64) if group_offsets is None else np.ascontiguousarray(group_offsets, dtype=np.int64)
        h = C.c_void_p()
        self._ctx.check(self._ctx._lib.pdbeda_list_blobs(self._h, _ptr(crs), len(crs), _ptr(off), len(off) - 1, C.byref(h)),
                        "pdbeda_list_blobs")
        return BlobList(self._ctx, h, self)

    def list_stats(self, crs):
        """Statistics of one explicit voxel set as a single blob (DensityBlob.fromCrsList).

        The set need not be connected: the per-component sums of the device job are
        combined here (a handful of rows)."""
        bl = self.list_blobs(crs)
        st = bl.stats()
        n = st["n"].astype(np.float64)
        tot = float(st["totalDensity"].sum())
        # a component whose own total density is 0 has no density-weighted centroid (0 / 0 on the device): it contributes
        # nothing to the weighted sum -- leaving it in would poison the whole centroid with NaN * 0
        w = st["totalDensity"]
        has = w != 0
        cen = (st["centroid"][has] * w[has, None]).sum(axis=0) / tot if (len(n) and tot != 0) else np.full(3, np.nan)
        cc = (st["coordCenter"] * n[:, None]).sum(axis=0) / n.sum() if len(n) else np.full(3, np.nan)
        return {"totalDensity": tot, "centroid": cen, "coordCenter": cc, "volume": float(st["volume"].sum()), "n": int(n.sum())}

    def region_sums(self, xyz, radii, group_offsets, cutoff):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        radii = np.ascontiguousarray(radii, dtype=np.float32)
        off = np.ascontiguousarray(group_offsets, dtype=np.int64)
        ng = len(off) - 1
        pos, neg = np.zeros(ng), np.zeros(ng)
        cnt = np.zeros(ng, dtype=np.int64)
        valid = np.zeros(ng, dtype=np.uint8)
        self._ctx.check(self._ctx._lib.pdbeda_region_sums(self._h, _ptr(xyz), _ptr(radii), len(xyz), _ptr(off), ng, C.c_float(cutoff),
                                                          _ptr(pos), _ptr(neg), _ptr(cnt), _ptr(valid)), "pdbeda_region_sums")
        return pos, neg, cnt, valid.astype(bool)

    def radial_profiles(self, xyz, radius, n_shells, cutoff):
        """pdbeda_radial_profiles: per atom, the voxels and the density of ``n_shells`` concentric shells out to ``radius``.
        A dict of (n_atoms, n_shells) arrays ``n``, ``sum``, ``nSig``, ``sumSig`` and the (n_atoms,) flags ``valid``."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        shape = (len(xyz), max(int(n_shells), 0))
        n, n_sig = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        total, total_sig = np.zeros(shape), np.zeros(shape)
        valid = np.zeros(len(xyz), dtype=np.uint8)
        self._ctx.check(self._ctx._lib.pdbeda_radial_profiles(self._h, _ptr(xyz), len(xyz), C.c_float(radius), int(n_shells), C.c_float(cutoff),
                                                              _ptr(n), _ptr(total), _ptr(n_sig), _ptr(total_sig), _ptr(valid)), "pdbeda_radial_profiles")
        return {"n": n, "sum": total, "nSig": n_sig, "sumSig": total_sig, "valid": valid.astype(bool)}

    def partition(self, xyz, max_distance, cutoff, owners=False):
        """pdbeda_map_partition: every voxel of the non-repeating box to its nearest atom within ``max_distance`` (or to nobody).
        A dict of (n_atoms,) arrays ``n``, ``sum``, ``nPos``, ``sumPos``, ``nNeg``, ``sumNeg``, the unowned totals ``unownedN`` (n, n_pos,
        n_neg) and ``unownedSum`` (sum, sum_pos, sum_neg, sum_sq) and, with ``owners``, the int32 volume ``owner`` (-1 = unowned)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        na = len(xyz)
        out = {"n": np.zeros(na, np.int64), "sum": np.zeros(na), "nPos": np.zeros(na, np.int64), "sumPos": np.zeros(na),
               "nNeg": np.zeros(na, np.int64), "sumNeg": np.zeros(na), "unownedN": np.zeros(3, np.int64), "unownedSum": np.zeros(4)}
        owner = np.full(self.unique_shape, -1, dtype=np.int32) if owners else None
        self._ctx.check(self._ctx._lib.pdbeda_map_partition(self._h, _ptr(xyz) if na else None, na, C.c_float(max_distance), C.c_float(cutoff),
                                                            _ptr(out["n"]), _ptr(out["sum"]), _ptr(out["nPos"]), _ptr(out["sumPos"]), _ptr(out["nNeg"]),
                                                            _ptr(out["sumNeg"]), _ptr(out["unownedN"]), _ptr(out["unownedSum"]),
                                                            _ptr(owner) if owners else None), "pdbeda_map_partition")
        if owners:
            out["owner"] = owner
        return out

    def interp_density(self, xyz):
        """pdbeda_interp_density: the trilinear density at arbitrary coordinates -> ((n,) float64 values, (n,) bool flags: all eight
        corners of the point are stored)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out, valid = np.zeros(len(xyz)), np.zeros(len(xyz), dtype=np.uint8)
        self._ctx.check(self._ctx._lib.pdbeda_interp_density(self._h, _ptr(xyz) if len(xyz) else None, len(xyz), _ptr(out), _ptr(valid)), "pdbeda_interp_density")
        return out, valid.astype(bool)

    def qscores(self, xyz, scored, step, ref, unit_pts, level_offsets, min_points):
        """pdbeda_atom_qscores: ``xyz`` are the atoms that compete for space, ``scored`` the indices of those to score (None: all, in
        order), ``ref`` the reference profile (one value per shell, shell k at radius k * float32(step)), ``unit_pts`` /
        ``level_offsets`` the candidate directions by level.  A dict of the (n_scored,) arrays ``q``, ``nPoints``, ``valid``, the
        (n_scored, n_shells) arrays ``shellN`` / ``shellMean`` and ``counters`` (atoms that overflowed the staging buffer, largest
        neighbour count)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        if scored is not None:
            scored = np.ascontiguousarray(scored, dtype=np.int32).reshape(-1)
        ref = np.ascontiguousarray(ref, dtype=np.float64).reshape(-1)
        unit = np.ascontiguousarray(unit_pts, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(level_offsets, dtype=np.int32).reshape(-1)
        if len(off) < 2 or len(unit) < int(off.max()):
            raise ValueError("level_offsets must name at least one level inside unit_pts")
        ns, shells = (len(xyz) if scored is None else len(scored)), len(ref)
        out = {"q": np.full(ns, np.nan), "nPoints": np.zeros(ns, np.int32), "shellN": np.zeros((ns, shells), np.int32), "shellMean": np.zeros((ns, shells)),
               "valid": np.zeros(ns, np.uint8), "counters": np.zeros(2, np.int64)}
        if ns == 0:      # (nothing to score: the library would touch nothing; an empty ``scored`` must never read as "all")
            out["valid"] = out["valid"].astype(bool)
            return out
        self._ctx.check(self._ctx._lib.pdbeda_atom_qscores(self._h, _ptr(xyz) if len(xyz) else None, len(xyz), _ptr(scored), ns, C.c_float(step), shells, _ptr(ref),
                                                           _ptr(unit), _ptr(off), len(off) - 1, int(min_points), _ptr(out["q"]), _ptr(out["nPoints"]),
                                                           _ptr(out["shellN"]), _ptr(out["shellMean"]), _ptr(out["valid"]), _ptr(out["counters"])), "pdbeda_atom_qscores")
        out["valid"] = out["valid"].astype(bool)
        return out

    def aggregate_cloud(self, xyz, radius, weight, residue, alias, key, bonded_off, bonded, owner_key, cutoff, min_cloud_electrons):
        """pdbeda_aggregate_cloud: everything of aggregateCloud that touches voxels, in one call.  Returns a dict of arrays:
        atoms (eligible index, totalDensity, voxels, centroid, distance), residue / domain cloud rows, owner states, totals."""
        lib, ctx = self._ctx._lib, self._ctx
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        arrs = {"radius": np.ascontiguousarray(radius, dtype=np.float32), "weight": np.ascontiguousarray(weight, dtype=np.float64),
                "residue": np.ascontiguousarray(residue, dtype=np.int32), "alias": np.ascontiguousarray(alias, dtype=np.int32),
                "key": np.ascontiguousarray(key, dtype=np.int32), "bonded_off": np.ascontiguousarray(bonded_off, dtype=np.int64),
                "bonded": np.ascontiguousarray(bonded, dtype=np.int32), "owner_key": np.ascontiguousarray(owner_key, dtype=np.int32)}
        n = len(xyz)
        assert all(len(arrs[k]) == n for k in ("radius", "weight", "residue", "alias", "key"))
        at = CloudAtoms(n, xyz.ctypes.data, *[arrs[k].ctypes.data for k in ("radius", "weight", "residue", "alias", "key")],
                        len(arrs["bonded_off"]) - 1, arrs["bonded_off"].ctypes.data, arrs["bonded"].ctypes.data,
                        len(arrs["owner_key"]), arrs["owner_key"].ctypes.data)
        h = C.c_void_p()
        ctx.check(lib.pdbeda_aggregate_cloud(self._h, C.byref(at), C.c_float(cutoff), C.c_double(min_cloud_electrons), C.byref(h)), "pdbeda_aggregate_cloud")
        try:
            counts, totals = np.zeros(4, np.int64), np.zeros(4, np.float64)
            ctx.check(lib.pdbeda_cloud_counts(h, _ptr(counts), _ptr(totals)), "pdbeda_cloud_counts")
            na, nr, nd, no = (int(v) for v in counts)
            out = {"numVoxels": int(totals[0]), "totalElectrons": float(totals[1]), "totalDensity": float(totals[2]), "centroidDistanceCutoff": float(totals[3]),
                   "atom": np.zeros(na, np.int32), "atom_total": np.zeros(na), "atom_n": np.zeros(na, np.int64), "atom_centroid": np.zeros((na, 3)),
                   "atom_distance": np.zeros(na), "owner_state": np.zeros(no, np.uint8)}
            ctx.check(lib.pdbeda_cloud_atom_rows(h, _ptr(out["atom"]), _ptr(out["atom_total"]), _ptr(out["atom_n"]), _ptr(out["atom_centroid"]),
                                                 _ptr(out["atom_distance"])), "pdbeda_cloud_atom_rows")
            for tag, cnt, fn in (("res", nr, lib.pdbeda_cloud_residue_rows), ("dom", nd, lib.pdbeda_cloud_domain_rows)):
                t = {"residue": np.zeros(cnt, np.int32), "total": np.zeros(cnt), "n": np.zeros(cnt, np.int64), "electrons": np.zeros(cnt), "centroid": np.zeros((cnt, 3))}
                ctx.check(fn(h, _ptr(t["residue"]), _ptr(t["total"]), _ptr(t["n"]), _ptr(t["electrons"]), _ptr(t["centroid"])), "pdbeda_cloud_rows")
                out[tag] = t
            ctx.check(lib.pdbeda_cloud_owner_states(h, _ptr(out["owner_state"])), "pdbeda_cloud_owner_states")
        finally:
            lib.pdbeda_cloud_free(h)
        return out

    def test_overlap(self, a, b):
        crs = np.concatenate([np.asarray(a, np.int32).reshape(-1, 3), np.asarray(b, np.int32).reshape(-1, 3)])
        off = np.array([0, len(a), len(a) + len(b)], dtype=np.int64)
        return bool(self._ctx.test_overlap(crs, off, [0], [1])[0])

    def free(self):
        if getattr(self, "_h", None) is not None and self._ctx._h:
            self._ctx._lib.pdbeda_map_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
