"""numpy restatement of the voxel-grid downsampling, shared by
tests/test_voxel_ref.py and tests/test_voxel_key.py (CPU) and
tests/test_gpu_voxel.py. The reference project has no such function, so this
is the checker.

Cells are exactly the operations of include/navgpu.h: np.floor((x - o) / v),
three separate IEEE operations. The order is np.unique's on the key
ix 2^42 + iy 2^21 + iz. A voxel's centroid is math.fsum (correctly rounded)
over its points divided by their number, and its centred sums are math.fsum of
the products of the rounded offsets from that centroid.

Tolerances, derived and not fitted. u = 2^-53, m a voxel's count, X the
largest |coordinate| among its points, v the voxel size.
  tol_c   = (m + 2) u X: a sum of m terms in any order is within
            (m - 1) u sum|x| <= (m - 1) u m X of the exact one, so the mean is
            within (m - 1) u X; its division rounds once more (u X); the
            restatement's own sum and division round twice (2 u X).
  tol_cov = m (2 v e + e^2 + u v^2) + m^2 u v^2 with e = u v + tol_c: an
            offset x - c (at most v in size) carries the centroid's error and
            one rounding, e; a product of two of them is then within
            2 v e + e^2, and rounds once, u v^2; m of them are added in any
            order, (m - 1) u m v^2.
Counts, cells, labels, the voxel count, stats[0..3] and the origin are
compared exactly.
"""
import math

import numpy as np

U = 2.0 ** -53
CELL_LIMIT = 2097152.0  # 2^21 cells per axis
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def cells_of(pts, voxel, origin):
    """(cells[n,3] int64, why[n]): why 0 kept, 1 non-finite, 2 out of range;
    the cell of a dropped point is (-1, -1, -1)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    o = np.asarray(origin, np.float64).reshape(3)
    finite = np.isfinite(pts).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((pts - o) / np.float64(voxel))
        inr = ((t >= 0.0) & (t < CELL_LIMIT)).all(1)
    why = np.where(finite, np.where(inr, 0, 2), 1)
    cells = np.full((len(pts), 3), -1, np.int64)
    cells[why == 0] = t[why == 0].astype(np.int64)
    return cells, why


def pack(cells):
    c = np.asarray(cells).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def keys_of(pts, voxel, origin):
    cells, why = cells_of(pts, voxel, origin)
    keys = np.full(len(cells), NO_KEY, np.uint64)
    keys[why == 0] = pack(cells[why == 0])
    return keys, cells, why


def default_origin(pts):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    fin = np.isfinite(pts).all(1)
    return pts[fin].min(0) if fin.any() else np.zeros(3)


def ref_voxel(pts, voxel, origin=None):
    """The restatement: a dict of nvox, centroids[m,3], counts[m], cov[m,6],
    cells[m,3], labels[n], stats[7] and, for the tolerances, X[m]."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    o = default_origin(pts) if origin is None else np.asarray(origin, np.float64).reshape(3)
    keys, cells, why = keys_of(pts, voxel, o)
    kept = np.flatnonzero(why == 0)
    uk, inv = np.unique(keys[kept], return_inverse=True)
    m = len(uk)
    labels = np.full(n, -1, np.int32)
    labels[kept] = inv
    counts = np.bincount(inv, minlength=m).astype(np.int32)
    order = kept[np.argsort(inv, kind="stable")]  # a voxel's points in ascending index
    start = np.concatenate([[0], np.cumsum(counts)])
    cen = np.zeros((m, 3))
    cov = np.zeros((m, 6))
    X = np.zeros(m)
    vcell = np.zeros((m, 3), np.int32)
    if m:
        first = order[start[:-1]]
        vcell[:] = cells[first]
        single = counts == 1
        cen[single] = pts[first[single]]
        X[single] = np.abs(pts[first[single]]).max(1)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        for j in np.flatnonzero(~single):
            P = pts[order[start[j]:start[j + 1]]]
            c = np.array([math.fsum(P[:, a]) / len(P) for a in range(3)])
            d = P - c
            cen[j] = c
            cov[j] = [math.fsum(d[:, a] * d[:, b]) for a, b in pairs]
            X[j] = np.abs(P).max()
    stats = np.array([m, len(kept), (why == 1).sum(), (why == 2).sum(), *o], np.float64)
    return {"nvox": m, "centroids": cen, "counts": counts, "cov": cov, "cells": vcell,
            "labels": labels, "stats": stats, "X": X}


def tolerances(counts, X, voxel):
    m = np.asarray(counts, np.float64)
    v = float(voxel)
    tol_c = (m + 2.0) * U * X
    e = U * v + tol_c
    tol_cov = m * (2.0 * v * e + e * e + U * v * v) + m * m * U * v * v
    return tol_c, tol_cov


def check_voxel(got, ref, voxel, what, cap=None):
    """got: a dict like ref_voxel's (keys that are absent or None are not
    compared; the voxel arrays hold the first min(nvox, cap) voxels). Prints
    the largest error over its tolerance before it asserts."""
    m = ref["nvox"]
    w = m if cap is None else min(m, cap)
    assert np.array_equal(got["stats"][:4], ref["stats"][:4]), (what, got["stats"], ref["stats"])
    assert (got["stats"][4:] == ref["stats"][4:]).all(), (what, got["stats"], ref["stats"])
    for name in ("counts", "cells"):
        if got.get(name) is not None:
            assert np.array_equal(got[name][:w], ref[name][:w]), (what, name)
    if got.get("labels") is not None:
        assert np.array_equal(got["labels"], ref["labels"]), (what, "labels")
    tol_c, tol_cov = tolerances(ref["counts"][:w], ref["X"][:w], voxel)
    ec = np.abs(got["centroids"][:w] - ref["centroids"][:w]).max(1) if w else np.zeros(0)
    msg = f"{what}: voxels {m} written {w}"
    if w:
        msg += f" centroid err/tol {np.max(ec / np.maximum(tol_c, 1e-300)):.3g}"
    assert (ec <= tol_c).all(), (what, "centroids")
    if got.get("cov") is not None:
        ev = np.abs(got["cov"][:w] - ref["cov"][:w]).max(1) if w else np.zeros(0)
        if w:
            msg += f" cov err/tol {np.max(ev / np.maximum(tol_cov, 1e-300)):.3g}"
        assert (ev <= tol_cov).all(), (what, "cov")
    print(msg)
