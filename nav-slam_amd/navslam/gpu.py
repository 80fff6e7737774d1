"""ctypes binding of libnavgpu.so (include/navgpu.h).

The HIP library is the product: if it is missing or the device is not a
gfx950 the constructor raises — there is no CPU fallback anywhere in this
package. Host-pointer calls take/return numpy arrays; device-pointer calls
take torch tensors (or raw integer addresses) already resident on the GPU.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.abspath(os.path.join(PKG, "..", "lib"))
# NAVGPU_LIB: an experimental build of the same library (A/B runs only)
LIBNAVGPU = os.environ.get("NAVGPU_LIB") or os.path.join(LIBDIR, "libnavgpu.so")

NAVGPU_OK = 0

_vp = C.c_void_p
_i32 = C.c_int32
_sz = C.c_size_t


class NavGpuError(RuntimeError):
    pass


def _declare(L):
    sig = {
        "navgpu_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
        "navgpu_destroy": (None, [_vp]),
        "navgpu_set_stream": (C.c_int, [_vp, _vp]),
        "navgpu_stream": (_vp, [_vp]),
        "navgpu_sync": (C.c_int, [_vp]),
        "navgpu_last_error": (C.c_char_p, []),
        "navgpu_version": (C.c_char_p, []),
        "navgpu_rows_max_cols": (C.c_int, []),
        "navgpu_curvature_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp]),
        "navgpu_curvature_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp]),
        "navgpu_project_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
        "navgpu_project_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
        "navgpu_transform_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
        "navgpu_kd_build_rows_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int,
                                               _vp, _vp, _vp, _vp]),
        "navgpu_kd_query_rows_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int,
                                               C.c_int, _vp, _vp, _vp]),
        "navgpu_kd_compact_rows_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int,
                                                 _vp, _vp, _vp, _vp, _vp]),
        "navgpu_kd_query_rows_lazy_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp,
                                                    C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
        "navgpu_kd_query_rows_lazy_corr_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp,
                                                         C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                                         _vp, _vp]),
        "navgpu_rows_corr_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                           C.c_int, _vp, _vp]),
        "navgpu_rows_corr_list_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int,
                                               C.c_int, _vp, _vp]),
        "navgpu_rows_match_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int,
                                            _vp, _vp, _vp, _vp]),
        "navgpu_rows_match_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int,
                                             _vp, _vp, _vp, _vp]),
        "navgpu_rows_match_batch_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                                  _vp, _vp, _vp, _vp]),
        "navgpu_knn_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.c_int, _vp, _vp]),
        "navgpu_knn_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.c_int, _vp, _vp]),
        "navgpu_pair_knn_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                          _vp, _vp, _vp, _vp]),
        "navgpu_align_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, C.c_int, C.c_double,
                                       _vp, _vp, _vp, _vp]),
        "navgpu_align_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, C.c_int, C.c_double,
                                        _vp, _vp, _vp, _vp]),
        "navgpu_transform_pose_dev": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
        "navgpu_icp_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.c_int, C.c_double, _vp, _vp,
                                     _vp, _vp]),
        "navgpu_icp_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.c_int, C.c_double, _vp, _vp,
                                      _vp, _vp]),
        "navgpu_normals_dev": (C.c_int, [_vp, _vp, _sz, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
        "navgpu_normals_host": (C.c_int, [_vp, _vp, _sz, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
        "navgpu_cloud_normals_dev": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _vp, _vp]),
        "navgpu_cloud_normals_host": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _vp, _vp]),
        "navgpu_align_plane_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp,
                                             C.c_int, C.c_double, C.c_double, _vp, _vp, _vp,
                                             _vp]),
        "navgpu_align_plane_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp,
                                              C.c_int, C.c_double, C.c_double, _vp, _vp, _vp,
                                              _vp]),
        "navgpu_icp_plane_dev": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, C.c_int,
                                           C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
        "navgpu_icp_plane_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.c_int, _vp, C.c_int,
                                            C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
        "navgpu_icp_plane_normals_host": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, C.c_int,
                                                    C.c_double, C.c_double, _vp, _vp, _vp,
                                                    _vp]),
        "navgpu_voxel_downsample_dev": (C.c_int, [_vp, _vp, _sz, C.c_double, _vp, _sz, _vp,
                                                  _vp, _vp, _vp, _vp, _vp]),
        "navgpu_voxel_downsample_host": (C.c_int, [_vp, _vp, _sz, C.c_double, _vp, _sz, _vp,
                                                   _vp, _vp, _vp, _vp, _vp]),
        "navgpu_kd_build_dev": (C.c_int, [_vp, _vp, _sz, C.c_int]),
        "navgpu_kd_build_host": (C.c_int, [_vp, _vp, _sz, C.c_int]),
        "navgpu_malloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
        "navgpu_free": (None, [_vp, _vp]),
        "navgpu_host_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
        "navgpu_host_free": (None, [_vp, _vp]),
        "navgpu_host_register": (C.c_int, [_vp, _vp, _sz]),
        "navgpu_host_unregister": (None, [_vp, _vp]),
        "navgpu_kd_rows_nodes_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_uint64,
                                               _vp, _vp]),
        "navgpu_upload": (C.c_int, [_vp, _vp, _vp, _sz]),
        "navgpu_download": (C.c_int, [_vp, _vp, _vp, _sz]),
        "navgpu_stream_copy_dev": (C.c_int, [_vp, _vp, _vp, _sz]),
        "navgpu_side_mark": (C.c_int, [_vp]),
        "navgpu_side_download": (C.c_int, [_vp, _vp, _vp, _sz]),
        "navgpu_timing_enable": (None, [_vp, C.c_int]),
        "navgpu_timing_select": (None, [_vp, C.c_char_p]),
        "navgpu_timing_read": (C.c_double, [_vp, C.c_char_p, C.c_int]),
        "navgpu_timing_count": (C.c_int, [_vp, C.c_char_p]),
        "navgpu_knn_fallbacks": (C.c_longlong, [_vp]),
        "navgpu_knn_overflows": (C.c_longlong, [_vp]),
        "navgpu_knn_check": (C.c_int, [_vp]),
        "navgpu_rows_tie_rows": (C.c_longlong, [_vp]),
        "navgpu_debug_nth_element": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return sig


_LIB = None


def load_library(path=LIBNAVGPU):
    """Load libnavgpu.so (raises if it was not built)."""
    global _LIB
    if _LIB is None:
        # Bind to the HIP runtime torch ships when torch is present: torch loads
        # its bundled libamdhip64 (SONAME libamdhip64.so.7) by path, so loading
        # /opt/rocm's copy first would leave two HSA runtimes in the process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise NavGpuError(
                f"{path} is missing: build it with `make -C nav-slam_amd` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        _LIB = C.CDLL(path)
        _declare(_LIB)
    return _LIB


def exported_symbols():
    """Names of every C entry point declared in include/navgpu.h."""
    L = load_library()
    return sorted(_declare(L).keys())


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


class NavGpu:
    """A libnavgpu context: device + stream + workspace."""

    def __init__(self, device=0, stream=None):
        self.L = load_library()
        h = _vp()
        self._check(self.L.navgpu_create(device, stream, C.byref(h)), "navgpu_create")
        self.h = h

    def _check(self, rc, what):
        if rc != NAVGPU_OK:
            msg = self.L.navgpu_last_error().decode(errors="replace")
            raise NavGpuError(f"{what} failed ({rc}): {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.L.navgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- plumbing
    def set_stream(self, stream_handle):
        self._check(self.L.navgpu_set_stream(self.h, stream_handle), "set_stream")

    def sync(self):
        self._check(self.L.navgpu_sync(self.h), "sync")

    @property
    def rows_max_cols(self):
        return self.L.navgpu_rows_max_cols()

    def timing(self, on=True):
        self.L.navgpu_timing_enable(self.h, 1 if on else 0)

    def timing_select(self, name=None):
        """Record only the region `name` while timing is on (None: all)."""
        self.L.navgpu_timing_select(self.h, None if name is None else name.encode())

    def stream_copy_dev(self, dst, src, nbytes):
        """Device-to-device copy by a plain streaming kernel (the measured HBM
        ceiling beside the roofline's peak; timed as "stream_copy")."""
        self._check(self.L.navgpu_stream_copy_dev(self.h, _ptr(dst), _ptr(src), nbytes),
                    "stream_copy_dev")

    def knn_fallbacks(self):
        """Queries of the last knn call that took the exact slow path (-1 if
        not recorded; set NAVGPU_KNN_STATS=1 before creating the context)."""
        return self.L.navgpu_knn_fallbacks(self.h)

    def knn_overflows(self):
        """k_knn tiles of the last knn call that overflowed the LDS tile and
        ran from global memory."""
        return self.L.navgpu_knn_overflows(self.h)

    def knn_check(self):
        """Raises NavGpuError (NAVGPU_EINTERNAL) when a k-NN kernel of the last
        knn call met an out-of-range index (synchronises)."""
        self._check(self.L.navgpu_knn_check(self.h), "knn_check")

    def rows_tie_rows(self):
        """Rows of the last rows_match call that had a distance tie and ran
        the reference tree (-1 if that call did not screen)."""
        return self.L.navgpu_rows_tie_rows(self.h)

    def debug_nth_element(self, key, perm, first, last, nth, block=False):
        """One reference nth_element as the per-row builds run it (device
        tensors: key f64 [n], perm int32 [n], permuted in place)."""
        self._check(self.L.navgpu_debug_nth_element(self.h, _ptr(key), _ptr(perm), len(perm),
                                                    first, last, nth, 1 if block else 0),
                    "debug_nth_element")

    def timing_read(self, name, reset=True):
        n = self.L.navgpu_timing_count(self.h, name.encode())
        ms = self.L.navgpu_timing_read(self.h, name.encode(), 1 if reset else 0)
        return ms, n

    # ---------------------------------------------------- host-pointer API
    def curvature(self, pts, want_curv=False):
        pts = np.ascontiguousarray(pts, np.float64)
        R, Cc = pts.shape[:2]
        mask = np.zeros((R, Cc), np.int32)
        curv = np.zeros((R, Cc)) if want_curv else None
        self._check(self.L.navgpu_curvature_host(self.h, _ptr(pts), R, Cc, _ptr(mask),
                                                 _ptr(curv)), "curvature")
        return (mask, curv) if want_curv else mask

    def project(self, depth):
        depth = np.ascontiguousarray(depth, np.int32)
        R, Cc = depth.shape
        out = np.zeros((R, Cc, 3))
        self._check(self.L.navgpu_project_host(self.h, _ptr(depth), R, Cc, _ptr(out)),
                    "project")
        return out

    def rows_match(self, src, tgt):
        src = np.ascontiguousarray(src, np.float64)
        tgt = np.ascontiguousarray(tgt, np.float64)
        R, Cc = src.shape[:2]
        sm = np.zeros((R, Cc), np.int32)
        tm = np.zeros((R, Cc), np.int32)
        idx = np.zeros((R, Cc), np.int32)
        dist = np.zeros((R, Cc))
        self._check(self.L.navgpu_rows_match_host(self.h, _ptr(src), _ptr(tgt), R, Cc,
                                                  _ptr(sm), _ptr(tm), _ptr(idx), _ptr(dist)),
                    "rows_match")
        return sm, tm, idx, dist

    def knn(self, tgt, queries, k):
        tgt = np.ascontiguousarray(tgt, np.float64).reshape(-1, 3)
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
        idx = np.zeros((len(q), k), np.int32)
        dist = np.zeros((len(q), k))
        self._check(self.L.navgpu_knn_host(self.h, _ptr(tgt), len(tgt), _ptr(q), len(q), k,
                                           _ptr(idx), _ptr(dist)), "knn")
        return idx, dist

    # marshalling shared by align, icp, align_plane and icp_plane
    @staticmethod
    def _cloud(pts):
        return np.ascontiguousarray(pts, np.float64).reshape(-1, 3)

    @staticmethod
    def _mask(mask, n, what):
        if mask is None:
            return None
        mask = np.ascontiguousarray(mask, np.int32).reshape(-1)
        if len(mask) != n:
            raise ValueError(what)
        return mask

    @staticmethod
    def _rows(idx, dist, nq, what):
        """rows of k slots per query as knn() returns them (an empty call has none)"""
        idx = np.ascontiguousarray(idx, np.int32).reshape((nq, -1) if nq else (0, 1))
        dist = np.ascontiguousarray(dist, np.float64).reshape((nq, -1) if nq else (0, 1))
        if idx.shape != dist.shape:
            raise ValueError(f"{what}: idx and dist differ in shape")
        return idx, dist

    @staticmethod
    def _target_normals(tgt, tgt_normals, tgt_curv, what):
        tn = np.ascontiguousarray(tgt_normals, np.float64).reshape(-1, 3)
        tc = np.ascontiguousarray(tgt_curv, np.float64).reshape(-1)
        if len(tn) != len(tgt) or len(tc) != len(tgt):
            raise ValueError(f"{what}: one normal and one curvature per target point")
        return tn, tc

    @staticmethod
    def _pose(init):
        """the 12 doubles (R row-major, then t) of init = (R, t); None: the identity"""
        pose = np.zeros(12)
        if init is None:
            pose[[0, 4, 8]] = 1.0
        else:
            pose[:9] = np.asarray(init[0], np.float64).reshape(9)
            pose[9:] = np.asarray(init[1], np.float64).reshape(3)
        return pose

    def align(self, src, tgt, idx, dist, max_dist=np.inf, mask=None):
        """One 6-DOF align step on the pairs (src[q], tgt[idx[q, 0]]) that pass
        the gate (navgpu.h): (R[3,3], t[3], stats[4]) with tgt ~ t + R src."""
        src, tgt = self._cloud(src), self._cloud(tgt)
        nq = len(src)
        idx, dist = self._rows(idx, dist, nq, "align")
        mask = self._mask(mask, nq, "align: one mask entry per query")
        R, t, stats = np.zeros((3, 3)), np.zeros(3), np.zeros(4)
        self._check(self.L.navgpu_align_host(
            self.h, _ptr(src), nq, _ptr(tgt), len(tgt), _ptr(idx), _ptr(dist), idx.shape[1],
            float(max_dist), _ptr(mask), _ptr(R), _ptr(t), _ptr(stats)), "align")
        return R, t, stats

    def icp(self, src, tgt, iters=10, max_dist=np.inf, mask=None, init=None):
        """Point-to-point ICP of src onto tgt, a fixed `iters` iterations from
        the pose init = (R, t) (default: the identity):
        (R[3,3], t[3], stats[iters,4], hist[iters,12])."""
        src, tgt = self._cloud(src), self._cloud(tgt)
        mask = self._mask(mask, len(src), "icp: one mask entry per source point")
        pose = self._pose(init)
        hist = np.zeros((iters, 12))
        stats = np.zeros((iters, 4))
        self._check(self.L.navgpu_icp_host(
            self.h, _ptr(src), len(src), _ptr(tgt), len(tgt), iters, float(max_dist),
            _ptr(mask), _ptr(pose), _ptr(hist), _ptr(stats)), "icp")
        return pose[:9].reshape(3, 3).copy(), pose[9:].copy(), stats, hist

    @staticmethod
    def _viewpoint(viewpoint):
        if viewpoint is None:
            return None
        return np.ascontiguousarray(viewpoint, np.float64).reshape(3)

    def normals(self, pts, k=8, viewpoint=None, idx=None):
        """Surface normals and curvatures of a cloud (navgpu.h): (normals[n,3],
        curv[n]). Neighbourhoods: the first k slots of the rows idx[n, stride]
        when given, else the cloud's own k-NN. A point without a plane gets the
        normal 0 and the curvature NaN."""
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        n = len(pts)
        vp = self._viewpoint(viewpoint)
        nrm, curv = np.zeros((n, 3)), np.zeros(n)
        if idx is None:
            self._check(self.L.navgpu_cloud_normals_host(
                self.h, _ptr(pts), n, k, _ptr(vp), _ptr(nrm), _ptr(curv)), "normals")
        else:
            idx = np.ascontiguousarray(idx, np.int32)
            if idx.ndim != 2 or len(idx) != n:
                raise ValueError("normals: idx is one row of neighbours per point")
            self._check(self.L.navgpu_normals_host(
                self.h, _ptr(pts), n, _ptr(idx), idx.shape[1], k, _ptr(vp), _ptr(nrm),
                _ptr(curv)), "normals")
        return nrm, curv

    def align_plane(self, src, tgt, tgt_normals, tgt_curv, idx, dist, max_dist=np.inf,
                    max_curv=np.inf, mask=None):
        """One point-to-plane step on the pairs (src[q], tgt[idx[q, 0]]) that
        pass the gate (navgpu.h): (R[3,3], t[3], stats[6])."""
        src, tgt = self._cloud(src), self._cloud(tgt)
        tn, tc = self._target_normals(tgt, tgt_normals, tgt_curv, "align_plane")
        nq = len(src)
        idx, dist = self._rows(idx, dist, nq, "align_plane")
        mask = self._mask(mask, nq, "align_plane: one mask entry per query")
        R, t, stats = np.zeros((3, 3)), np.zeros(3), np.zeros(6)
        self._check(self.L.navgpu_align_plane_host(
            self.h, _ptr(src), nq, _ptr(tgt), len(tgt), _ptr(tn), _ptr(tc), _ptr(idx),
            _ptr(dist), idx.shape[1], float(max_dist), float(max_curv), _ptr(mask), _ptr(R),
            _ptr(t), _ptr(stats)), "align_plane")
        return R, t, stats

    def icp_plane(self, src, tgt, tgt_normals=None, tgt_curv=None, iters=10, max_dist=np.inf,
                  max_curv=np.inf, mask=None, init=None, kn=8, viewpoint=None):
        """Point-to-plane ICP of src onto tgt, a fixed `iters` iterations from
        the pose init = (R, t) (default: the identity). The target's normals
        and curvatures are the given ones, or computed once from its kn-NN and
        `viewpoint` as normals() does:
        (R[3,3], t[3], stats[iters,6], hist[iters,12])."""
        src, tgt = self._cloud(src), self._cloud(tgt)
        mask = self._mask(mask, len(src), "icp_plane: one mask entry per source point")
        if (tgt_normals is None) != (tgt_curv is None):
            raise ValueError("icp_plane: give both tgt_normals and tgt_curv, or neither")
        pose = self._pose(init)
        hist = np.zeros((iters, 12))
        stats = np.zeros((iters, 6))
        if tgt_normals is None:
            vp = self._viewpoint(viewpoint)
            self._check(self.L.navgpu_icp_plane_host(
                self.h, _ptr(src), len(src), _ptr(tgt), len(tgt), kn, _ptr(vp), iters,
                float(max_dist), float(max_curv), _ptr(mask), _ptr(pose), _ptr(hist),
                _ptr(stats)), "icp_plane")
        else:
            tn, tc = self._target_normals(tgt, tgt_normals, tgt_curv, "icp_plane")
            self._check(self.L.navgpu_icp_plane_normals_host(
                self.h, _ptr(src), len(src), _ptr(tgt), len(tgt), _ptr(tn), _ptr(tc), iters,
                float(max_dist), float(max_curv), _ptr(mask), _ptr(pose), _ptr(hist),
                _ptr(stats)), "icp_plane")
        return pose[:9].reshape(3, 3).copy(), pose[9:].copy(), stats, hist

    def voxel_downsample(self, pts, voxel, origin=None, cov=False, cells=False, labels=False,
                         cap=None):
        """Voxel-grid downsampling of a cloud (navgpu.h): one point per occupied
        cell of edge `voxel`, in ascending key order. origin: 3 doubles, or None
        for the per-axis minimum of the finite points. Returns (centroids[m,3],
        counts[m], then cov[m,6], cells[m,3] and labels[n] where asked for,
        stats[7]), the voxel arrays trimmed to the m voxels. cap (default: the
        number of points) bounds m: more voxels than cap raise NavGpuError."""
        pts = self._cloud(pts)
        n = len(pts)
        cap = n if cap is None else int(cap)
        org = self._viewpoint(origin)
        cen = np.zeros((cap, 3))
        cnt = np.zeros(cap, np.int32)
        cv = np.zeros((cap, 6)) if cov else None
        ce = np.zeros((cap, 3), np.int32) if cells else None
        lab = np.zeros(n, np.int32) if labels else None
        stats = np.zeros(7)
        self._check(self.L.navgpu_voxel_downsample_host(
            self.h, _ptr(pts), n, float(voxel), _ptr(org), cap, _ptr(cen), _ptr(cnt), _ptr(cv),
            _ptr(ce), _ptr(lab), _ptr(stats)), "voxel_downsample")
        m = int(stats[0])
        out = [cen[:m], cnt[:m]]
        if cov:
            out.append(cv[:m])
        if cells:
            out.append(ce[:m])
        if labels:
            out.append(lab)
        return (*out, stats)

    def kd_build(self, pts, depth0=0):
        """Reference buildKDTree permutation of `pts` (returns a new array)."""
        p = np.array(pts, np.float64, order="C").reshape(-1, 3)
        self._check(self.L.navgpu_kd_build_host(self.h, _ptr(p), len(p), depth0),
                    "kd_build")
        return p

    # -------------------------------------------------- device-pointer API
    def curvature_dev(self, pts, R, Cc, mask, curv=None):
        self._check(self.L.navgpu_curvature_dev(self.h, _ptr(pts), R, Cc, _ptr(mask),
                                                _ptr(curv)), "curvature_dev")

    def transform_dev(self, pts, n, Rm, t, tr, out, out_last=None):
        Rm = np.ascontiguousarray(Rm, np.float64)
        t = np.ascontiguousarray(t, np.float64)
        tr = None if tr is None else np.ascontiguousarray(tr, np.float64)
        self._check(self.L.navgpu_transform_dev(self.h, _ptr(pts), n, _ptr(Rm), _ptr(t),
                                                _ptr(tr), _ptr(out), _ptr(out_last)),
                    "transform_dev")

    def align_dev(self, src, nq, tgt, nt, idx, dist, stride, max_dist, mask, delta, pose,
                  stats):
        self._check(self.L.navgpu_align_dev(
            self.h, _ptr(src), nq, _ptr(tgt), nt, _ptr(idx), _ptr(dist), stride,
            float(max_dist), _ptr(mask), _ptr(delta), _ptr(pose), _ptr(stats)), "align_dev")

    def transform_pose_dev(self, pts, n, pose, out):
        """transform_dev with the 12-double pose (R row-major, then t) on the device."""
        self._check(self.L.navgpu_transform_pose_dev(self.h, _ptr(pts), n, _ptr(pose),
                                                     _ptr(out)), "transform_pose_dev")

    def icp_dev(self, src, nq, tgt, nt, iters, max_dist, mask, pose, hist=None, stats=None):
        self._check(self.L.navgpu_icp_dev(
            self.h, _ptr(src), nq, _ptr(tgt), nt, iters, float(max_dist), _ptr(mask),
            _ptr(pose), _ptr(hist), _ptr(stats)), "icp_dev")

    def normals_dev(self, pts, n, idx, stride, k, viewpoint, normals, curv=None):
        """viewpoint: 3 host doubles or None; the rest device pointers."""
        vp = self._viewpoint(viewpoint)
        self._check(self.L.navgpu_normals_dev(self.h, _ptr(pts), n, _ptr(idx), stride, k,
                                              _ptr(vp), _ptr(normals), _ptr(curv)),
                    "normals_dev")

    def cloud_normals_dev(self, pts, n, k, viewpoint, normals, curv=None):
        vp = self._viewpoint(viewpoint)
        self._check(self.L.navgpu_cloud_normals_dev(self.h, _ptr(pts), n, k, _ptr(vp),
                                                    _ptr(normals), _ptr(curv)),
                    "cloud_normals_dev")

    def align_plane_dev(self, src, nq, tgt, nt, tgt_normals, tgt_curv, idx, dist, stride,
                        max_dist, max_curv, mask, delta, pose, stats):
        self._check(self.L.navgpu_align_plane_dev(
            self.h, _ptr(src), nq, _ptr(tgt), nt, _ptr(tgt_normals), _ptr(tgt_curv), _ptr(idx),
            _ptr(dist), stride, float(max_dist), float(max_curv), _ptr(mask), _ptr(delta),
            _ptr(pose), _ptr(stats)), "align_plane_dev")

    def icp_plane_dev(self, src, nq, tgt, nt, tgt_normals, tgt_curv, iters, max_dist, max_curv,
                      mask, pose, hist=None, stats=None):
        self._check(self.L.navgpu_icp_plane_dev(
            self.h, _ptr(src), nq, _ptr(tgt), nt, _ptr(tgt_normals), _ptr(tgt_curv), iters,
            float(max_dist), float(max_curv), _ptr(mask), _ptr(pose), _ptr(hist), _ptr(stats)),
            "icp_plane_dev")

    def voxel_downsample_dev(self, pts, n, voxel, origin, cap, centroids, counts, cov, cells,
                             labels, stats):
        """origin: 3 host doubles or None; the rest device pointers (counts,
        cov, cells and labels may be None)."""
        org = self._viewpoint(origin)
        self._check(self.L.navgpu_voxel_downsample_dev(
            self.h, _ptr(pts), n, float(voxel), _ptr(org), cap, _ptr(centroids), _ptr(counts),
            _ptr(cov), _ptr(cells), _ptr(labels), _ptr(stats)), "voxel_downsample_dev")

    def kd_build_dev(self, pts, n, depth0=0):
        self._check(self.L.navgpu_kd_build_dev(self.h, _ptr(pts), n, depth0), "kd_build_dev")

    def kd_build_rows_dev(self, feat_src, coords, R, Cc, tree_pts, tree_col, tree_n,
                          mask=None):
        self._check(self.L.navgpu_kd_build_rows_dev(
            self.h, _ptr(feat_src), _ptr(coords), R, Cc, _ptr(tree_pts), _ptr(tree_col),
            _ptr(tree_n), _ptr(mask)), "kd_build_rows_dev")

    def kd_rows_nodes_dev(self, tree_pts, tree_n, R, Cc, host_base, nodes, row_off):
        self._check(self.L.navgpu_kd_rows_nodes_dev(
            self.h, _ptr(tree_pts), _ptr(tree_n), R, Cc, int(host_base), _ptr(nodes),
            _ptr(row_off)), "kd_rows_nodes_dev")

    def kd_query_rows_dev(self, tree_pts, tree_n, feat_src, queries, R, Cc, nn_pos,
                          nn_dist, mask=None):
        self._check(self.L.navgpu_kd_query_rows_dev(
            self.h, _ptr(tree_pts), _ptr(tree_n), _ptr(feat_src), _ptr(queries), R, Cc,
            _ptr(nn_pos), _ptr(nn_dist), _ptr(mask)), "kd_query_rows_dev")

    def kd_compact_rows_dev(self, feat_src, coords, R, Cc, tree_pts, tree_col, tree_n,
                            mask=None, built=None):
        self._check(self.L.navgpu_kd_compact_rows_dev(
            self.h, _ptr(feat_src), _ptr(coords), R, Cc, _ptr(tree_pts), _ptr(tree_col),
            _ptr(tree_n), _ptr(mask), _ptr(built)), "kd_compact_rows_dev")

    def kd_query_rows_lazy_dev(self, tree_pts, tree_col, tree_n, feat_src, queries, R, Cc,
                               nn_pos, nn_dist, mask=None, built=None):
        self._check(self.L.navgpu_kd_query_rows_lazy_dev(
            self.h, _ptr(tree_pts), _ptr(tree_col), _ptr(tree_n), _ptr(feat_src),
            _ptr(queries), R, Cc, _ptr(nn_pos), _ptr(nn_dist), _ptr(mask), _ptr(built)),
            "kd_query_rows_lazy_dev")

    def kd_query_rows_lazy_corr_dev(self, tree_pts, tree_col, tree_n, feat_src, queries, R, Cc,
                                    nn_pos, nn_dist, mask, built, ori, sums):
        self._check(self.L.navgpu_kd_query_rows_lazy_corr_dev(
            self.h, _ptr(tree_pts), _ptr(tree_col), _ptr(tree_n), _ptr(feat_src),
            _ptr(queries), R, Cc, _ptr(nn_pos), _ptr(nn_dist), _ptr(mask), _ptr(built),
            _ptr(ori), _ptr(sums)), "kd_query_rows_lazy_corr_dev")

    def rows_corr_dev(self, tree_pts, tree_n, nn_pos, nn_dist, ori, R, Cc, keep, sums):
        self._check(self.L.navgpu_rows_corr_dev(
            self.h, _ptr(tree_pts), _ptr(tree_n), _ptr(nn_pos), _ptr(nn_dist), _ptr(ori),
            R, Cc, _ptr(keep), _ptr(sums)), "rows_corr")

    def rows_corr_list_dev(self, tree_pts, tree_n, nn_pos, nn_dist, ori, R, Cc, lst, count):
        self._check(self.L.navgpu_rows_corr_list_dev(
            self.h, _ptr(tree_pts), _ptr(tree_n), _ptr(nn_pos), _ptr(nn_dist), _ptr(ori), R, Cc,
            _ptr(lst), _ptr(count)), "rows_corr_list_dev")

    def rows_match_dev(self, src, tgt, R, Cc, src_mask, tgt_mask, nn_idx, nn_dist):
        self._check(self.L.navgpu_rows_match_dev(
            self.h, _ptr(src), _ptr(tgt), R, Cc, _ptr(src_mask), _ptr(tgt_mask),
            _ptr(nn_idx), _ptr(nn_dist)), "rows_match_dev")

    def rows_match_batch_dev(self, src, tgt, npairs, R, Cc, src_mask, tgt_mask, nn_idx,
                             nn_dist):
        self._check(self.L.navgpu_rows_match_batch_dev(
            self.h, _ptr(src), _ptr(tgt), npairs, R, Cc, _ptr(src_mask), _ptr(tgt_mask),
            _ptr(nn_idx), _ptr(nn_dist)), "rows_match_batch_dev")

    def knn_dev(self, tgt, nt, queries, nq, k, idx, dist):
        self._check(self.L.navgpu_knn_dev(self.h, _ptr(tgt), nt, _ptr(queries), nq, k,
                                          _ptr(idx), _ptr(dist)), "knn_dev")

    def pair_knn_dev(self, src, tgt, R, Cc, k, src_mask, tgt_mask, idx, dist):
        self._check(self.L.navgpu_pair_knn_dev(
            self.h, _ptr(src), _ptr(tgt), R, Cc, k, _ptr(src_mask), _ptr(tgt_mask),
            _ptr(idx), _ptr(dist)), "pair_knn_dev")
