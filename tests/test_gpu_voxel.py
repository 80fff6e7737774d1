"""Voxel-grid downsampling on the GPU (voxel.hip) against the numpy
restatement of tests/voxel_ref.py, whose docstring derives the tolerances. The
reference project has no such function, so the restatement is the checker.
Every case runs through navgpu_voxel_downsample_dev and _host unless noted.
Counts, cells, labels, the voxel count, stats[0..3] and the origin are compared
exactly; centroids and the centred sums within tol_c and tol_cov.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from reg_ref import l9_clouds
from voxel_ref import check_voxel, ref_voxel

pytestmark = pytest.mark.gpu

# k_vox_hist / k_vox_scatter: one tile of 256 threads x 4 keys per block
VOX_SORT_TILE = 1024
# k_vox_heads, k_vox_number, k_vox_seg_agg / _out: one sorted position per thread
VOX_SEG_TILE = 256
# k_vox_setup's loop over k_vox_min's rows (256 a trip), and the size from which
# a thread of k_vox_scan_sums and k_vox_seg_carry takes more than one tile's sum
VOX_SEG_ONE_TRIP = 256 * VOX_SEG_TILE
# k_vox_offsets (256 tiles a trip) and k_vox_min (at most 1024 blocks of 256
# threads, one point per thread and trip)
VOX_SORT_ONE_TRIP = 256 * VOX_SORT_TILE
VOX_MIN_ONE_TRIP = 1024 * 256

NAVGPU_EINVAL, NAVGPU_ERANGE = -1, -4
ORIGIN = (-3.5, 0.0, 12.25)
SENTINEL = 7


@pytest.fixture(scope="module")
def gpu():
    from navslam.gpu import NavGpu
    g = NavGpu(0)
    yield g
    g.close()


def _addr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _buffers(n, cap, pad, want):
    """output arrays with `pad` sentinel voxels behind cap"""
    w = cap + pad
    return {"centroids": np.full((w, 3), float(SENTINEL)),
            "counts": np.full(w, SENTINEL, np.int32) if "counts" in want else None,
            "cov": np.full((w, 6), float(SENTINEL)) if "cov" in want else None,
            "cells": np.full((w, 3), SENTINEL, np.int32) if "cells" in want else None,
            "labels": np.full(n, SENTINEL, np.int32) if "labels" in want else None,
            "stats": np.full(7, float(SENTINEL))}


ALL = ("counts", "cov", "cells", "labels")


def run_host(gpu, pts, voxel, origin, cap=None, pad=0, want=ALL):
    """navgpu_voxel_downsample_host: (status, outputs)"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    cap = n if cap is None else cap
    o = _buffers(n, cap, pad, want)
    org = None if origin is None else np.ascontiguousarray(origin, np.float64)
    rc = gpu.L.navgpu_voxel_downsample_host(
        gpu.h, _addr(pts), n, float(voxel), _addr(org), cap, _addr(o["centroids"]),
        _addr(o["counts"]), _addr(o["cov"]), _addr(o["cells"]), _addr(o["labels"]),
        _addr(o["stats"]))
    return rc, o


def run_dev(gpu, pts, voxel, origin, cap=None, pad=0, want=ALL):
    """navgpu_voxel_downsample_dev on device tensors: (status, outputs)"""
    import torch
    dev = torch.device("cuda", 0)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    cap = n if cap is None else cap
    host = _buffers(n, cap, pad, want)
    d = {k: None if v is None else torch.from_numpy(v).to(dev) for k, v in host.items()}
    d_pts = torch.from_numpy(pts).to(dev) if n else None
    org = None if origin is None else np.ascontiguousarray(origin, np.float64)
    torch.cuda.synchronize()

    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())
    rc = gpu.L.navgpu_voxel_downsample_dev(
        gpu.h, ptr(d_pts), n, float(voxel), _addr(org), cap, ptr(d["centroids"]),
        ptr(d["counts"]), ptr(d["cov"]), ptr(d["cells"]), ptr(d["labels"]), ptr(d["stats"]))
    gpu.sync()
    return rc, {k: None if v is None else v.cpu().numpy() for k, v in d.items()}


RUNNERS = {"dev": run_dev, "host": run_host}


def both(gpu, pts, voxel, origin, ref, what, **kw):
    """both entry points against ref; returns their outputs"""
    outs = {}
    for name, run in RUNNERS.items():
        rc, out = run(gpu, pts, voxel, origin, **kw)
        assert rc == 0, (what, name, rc)
        check_voxel(out, ref, voxel, f"{what} {name}")
        outs[name] = out
    return outs


_CLOUDS, _REFS = {}, {}


def cloud(n):
    """n points uniform in [0, 1000)^3, made once per size"""
    if n not in _CLOUDS:
        _CLOUDS[n] = np.random.default_rng(9000 + n).uniform(0.0, 1000.0, (n, 3))
    return _CLOUDS[n]


def cloud_ref(n, origin):
    if (n, origin) not in _REFS:
        _REFS[n, origin] = ref_voxel(cloud(n), 37.0, origin)
    return _REFS[n, origin]


# ------------------------------------------------------------------- 1 sizes
SIZES = [0, 1, 63, 64, 65,
         VOX_SEG_TILE - 1, VOX_SEG_TILE, VOX_SEG_TILE + 1,
         VOX_SORT_TILE - 1, VOX_SORT_TILE, VOX_SORT_TILE + 1,
         VOX_SEG_ONE_TRIP - 1, VOX_SEG_ONE_TRIP, VOX_SEG_ONE_TRIP + 1,
         70001,
         VOX_SORT_ONE_TRIP - 1, VOX_SORT_ONE_TRIP, VOX_SORT_ONE_TRIP + 1]
assert VOX_MIN_ONE_TRIP == VOX_SORT_ONE_TRIP  # one set of sizes covers both


@pytest.mark.parametrize("origin", [None, ORIGIN], ids=["min", "given"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n, origin):
    ref = cloud_ref(n, origin)
    both(gpu, cloud(n), 37.0, origin, ref, f"n={n} origin={origin}")


# ------------------------------------------------------------------- 2 faces
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), ORIGIN], ids=["zero", "offset"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_faces(gpu, axis, origin):
    o = np.array(origin)
    pts = np.tile(o + 0.05, (100, 1))
    pts[:, axis] = o[axis] + np.arange(100) * 0.1
    ref = ref_voxel(pts, 0.1, origin)
    assert 50 <= ref["nvox"] <= 100 and ref["stats"][1] == 100
    both(gpu, pts, 0.1, origin, ref, f"faces axis {axis}")


# --------------------------------------------------------------- 3 key range
def test_key_range_and_order(gpu):
    top = 2097151
    pts = []
    for a in range(3):
        for x in (top + 0.5, top + 1.0, -0.5):
            p = [0.5, 0.5, 0.5]
            p[a] = x
            pts.append(p)
    pts.append([top + 0.5] * 3)                       # every key bit
    pts += [[1048579.5, 7.5, 7.5], [3.5, 7.5, 7.5]]   # differ in ix alone, in the top digit
    pts += [[9.5, 9.5, 5.5], [9.5, 9.5, 4.5]]         # differ in the lowest bit of iz
    pts = np.array(pts)
    origin = (0.0, 0.0, 0.0)
    ref = ref_voxel(pts, 1.0, origin)
    assert ref["stats"][:4].tolist() == [8.0, 8.0, 0.0, 6.0]
    outs = both(gpu, pts, 1.0, origin, ref, "key range")
    for out in outs.values():
        assert out["labels"].tolist() == [6, -1, -1, 1, -1, -1, 0, -1, -1, 7, 5, 2, 4, 3]
        assert out["cells"][:8].tolist() == [
            [0, 0, top], [0, top, 0], [3, 7, 7], [9, 9, 4], [9, 9, 5], [1048579, 7, 7],
            [top, 0, 0], [top, top, top]]


# --------------------------------------------------------------- 4 non-finite
def _with_bad_points(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, 1000.0, (n + 9, 3))
    where = rng.choice(n + 9, 9, replace=False)
    bad = [(a, x) for a in range(3) for x in (np.nan, np.inf, -np.inf)]
    for i, (a, x) in zip(where, bad):
        pts[i] = -5000.0      # would move the origin if the point counted
        pts[i, a] = x
    return pts, where


def test_non_finite_points_are_dropped(gpu):
    pts, where = _with_bad_points(1000, 41)
    ref = ref_voxel(pts, 37.0)
    assert ref["stats"][1:4].tolist() == [1000.0, 9.0, 0.0] and (ref["stats"][4:] >= 0.0).all()
    outs = both(gpu, pts, 37.0, None, ref, "non-finite")
    for out in outs.values():
        assert (out["labels"][where] == -1).all()
    only = pts[where]
    ref = ref_voxel(only, 37.0)
    assert ref["nvox"] == 0 and ref["stats"].tolist() == [0.0, 0.0, 9.0, 0.0, 0.0, 0.0, 0.0]
    both(gpu, only, 37.0, None, ref, "only non-finite")


# ---------------------------------------------------------------- 5 one voxel
def test_one_voxel_holds_every_point(gpu):
    pts = np.random.default_rng(5).uniform(0.0, 1.0, (70001, 3))
    origin = (0.0, 0.0, 0.0)
    ref = ref_voxel(pts, 1.0, origin)
    assert ref["nvox"] == 1 and ref["counts"].tolist() == [70001]
    both(gpu, pts, 1.0, origin, ref, "one voxel")


# -------------------------------------------------------------- 6 all distinct
def test_all_distinct_lattice(gpu):
    g = np.arange(16)
    ix, iy, iz = np.meshgrid(g, g, g, indexing="ij")
    lattice = (np.stack([ix, iy, iz], -1).reshape(-1, 3) + 0.5) * 2.0
    perm = np.random.default_rng(6).permutation(4096)
    pts = lattice[perm]
    origin = (0.0, 0.0, 0.0)
    ref = ref_voxel(pts, 2.0, origin)
    assert ref["nvox"] == 4096
    outs = both(gpu, pts, 2.0, origin, ref, "lattice")
    for out in outs.values():
        assert (out["counts"] == 1).all()
        assert out["centroids"].tobytes() == lattice.tobytes()      # bit for bit
        assert out["cov"].tobytes() == np.zeros((4096, 6)).tobytes()
        assert np.array_equal(out["labels"], perm)                  # the inverse of the sort
        assert np.array_equal(out["centroids"][out["labels"]], pts)


# ---------------------------------------------------------------- 7 room scan
def check_room(out, pts, voxel):
    m = int(out["stats"][0])
    lab = out["labels"]
    assert np.array_equal(out["counts"][:m], np.bincount(lab[lab >= 0], minlength=m))
    lo = out["stats"][4:] + out["cells"][lab] * voxel
    inside = (pts >= lo - 1e-9 * voxel) & (pts < lo + voxel * (1 + 1e-9))
    assert inside[lab >= 0].all()


def test_room_scan(gpu):
    _, tgt = l9_clouds()
    ref = ref_voxel(tgt, 100.0)
    assert ref["nvox"] == 3961 and ref["counts"].max() == 81
    assert ref["cells"].max(0).tolist() == [161, 122, 40]
    outs = both(gpu, tgt, 100.0, None, ref, "room")
    for out in outs.values():
        assert int(out["stats"][0]) == 3961 and out["counts"][:3961].max() == 81
        assert out["cells"][:3961].max(0).tolist() == [161, 122, 40]
        j = int(np.argmax(out["counts"][:3961]))                    # the zero-filled dropouts
        assert out["centroids"][j].tolist() == [0.0, 0.0, 0.0]
        check_room(out, tgt, 100.0)


# ----------------------------------------------------------------- 8 capacity
def test_capacity_clamps_and_flags(gpu):
    pts, ref = cloud(70001), cloud_ref(70001, None)
    cap, pad = ref["nvox"] // 2, 64
    assert cap > 1000
    for name, run in RUNNERS.items():
        rc, out = run(gpu, pts, 37.0, None, cap=cap, pad=pad)
        assert rc == (NAVGPU_ERANGE if name == "host" else 0), name
        assert out["stats"][0] == ref["nvox"]
        check_voxel(out, ref, 37.0, f"capacity {name}", cap=cap)    # labels: the true numbers
        assert out["labels"].max() == ref["nvox"] - 1
        for k in ("centroids", "counts", "cov", "cells"):
            assert (out[k][cap:] == SENTINEL).all(), (name, k)
    msg = gpu.L.navgpu_last_error().decode()
    assert "capacity" in msg


# ------------------------------------------------------------- 9 large offset
def test_large_offset(gpu):
    _, tgt = l9_clouds()
    pts = tgt + np.array([1e7, -2e7, 3e6])
    ref = ref_voxel(pts, 100.0)
    assert ref["X"].max() > 1e7
    both(gpu, pts, 100.0, None, ref, "large offset")


# ------------------------------------------------------------- 10 determinism
def test_voxel_deterministic(gpu):
    from navslam.gpu import NavGpu
    pts, _ = _with_bad_points(70001 - 9, 10)
    assert len(pts) == 70001
    runs = [run_dev(gpu, pts, 37.0, None)[1], run_dev(gpu, pts, 37.0, None)[1],
            run_host(gpu, pts, 37.0, None)[1]]
    g2 = NavGpu(0)
    try:
        runs.append(run_dev(g2, pts, 37.0, None)[1])
    finally:
        g2.close()
    m = int(runs[0]["stats"][0])
    assert m > 10000
    for other in runs[1:]:
        for k, v in runs[0].items():
            w = v if k in ("labels", "stats") else v[:m]
            o = other[k] if k in ("labels", "stats") else other[k][:m]
            assert w.tobytes() == o.tobytes(), k


# --------------------------------------------------------------- 11 arguments
@pytest.mark.parametrize("runner", ["dev", "host"])
def test_bad_arguments(gpu, runner):
    pts = cloud(257)
    for voxel in (0.0, -1.0, np.nan, np.inf):
        rc, out = RUNNERS[runner](gpu, pts, voxel, None)
        assert rc == NAVGPU_EINVAL, voxel
        assert (out["stats"] == SENTINEL).all() and (out["centroids"] == SENTINEL).all()
    for origin in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        rc, out = RUNNERS[runner](gpu, pts, 37.0, origin)
        assert rc == NAVGPU_EINVAL, origin
        assert (out["stats"] == SENTINEL).all()
    # n is checked before anything is read or launched: 2^31 points are out of range
    few, stats = np.zeros((4, 3)), np.full(7, float(SENTINEL))
    entry = getattr(gpu.L, f"navgpu_voxel_downsample_{runner}")
    rc = entry(gpu.h, None, 2 ** 31, 1.0, None, 4, _addr(few), None, None, None, None,
               _addr(stats))
    assert rc == NAVGPU_ERANGE and (stats == SENTINEL).all() and (few == 0.0).all()


@pytest.mark.parametrize("runner", ["dev", "host"])
def test_nullable_outputs_in_every_combination(gpu, runner):
    pts, ref = cloud(1025), cloud_ref(1025, ORIGIN)
    for r in range(len(ALL) + 1):
        for want in itertools.combinations(ALL, r):
            rc, out = RUNNERS[runner](gpu, pts, 37.0, ORIGIN, want=want)
            assert rc == 0, want
            assert [k for k in ALL if out[k] is not None] == list(want)
            check_voxel(out, ref, 37.0, f"{runner} outputs {want}")


def test_numpy_method(gpu):
    pts, ref = cloud(1025), cloud_ref(1025, None)
    cen, cnt, stats = gpu.voxel_downsample(pts, 37.0)
    assert cen.shape == (ref["nvox"], 3) and cnt.shape == (ref["nvox"],)
    check_voxel({"centroids": cen, "counts": cnt, "stats": stats}, ref, 37.0, "method")
    cen, cnt, cov, cells, labels, stats = gpu.voxel_downsample(
        pts, 37.0, cov=True, cells=True, labels=True)
    check_voxel({"centroids": cen, "counts": cnt, "cov": cov, "cells": cells, "labels": labels,
                 "stats": stats}, ref, 37.0, "method, every output")
    from navslam.gpu import NavGpuError
    with pytest.raises(NavGpuError):
        gpu.voxel_downsample(pts, 37.0, cap=ref["nvox"] - 1)
