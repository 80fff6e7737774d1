"""Surface normals, the point-to-plane step and its ICP loop on the GPU
(plane.hip) against the numpy restatements of tests/reg_ref.py. The
reference project has none of this, so the restatements are the checkers.

Normals: with l0 <= l1 <= l2 the eigenvalues of the centred covariance, the
eigenvector of l0 moves by |dC| / (l1 - l0) under a perturbation dC, and the
centred second pass leaves |dC| <= eps (l2 + max|coord| sqrt(l2)) up to a
small factor, so tol_n = 1024 eps (1 + max|coord| / sqrt(l2)) l2 / (l1 - l0)
and tol_curv = 1024 eps (1 + max|coord| / sqrt(l2)). A point is compared only
where (l1 - l0) / l2 >= 1e-6; the valid / invalid split is compared exactly
everywhere. The step's tolerances are ref_plane's (from eps, cond_2(S) and the
data's magnitudes).
"""
import numpy as np
import pytest

from reg_ref import (EPS, apply_pose, check_step, knn_numpy, l9_clouds, ref_normals, ref_plane,
                     rot, strided)

pytestmark = pytest.mark.gpu

# k_normals: at most 1024 blocks of 256 threads, one point per thread and trip
NORM_ONE_TRIP = 1024 * 256
# the plane step's moments kernel: at most 1024 blocks of 256 threads, 2 queries per thread and trip
PLANE_ONE_TRIP = 1024 * 256 * 2


@pytest.fixture(scope="module")
def gpu():
    from navslam.gpu import NavGpu
    g = NavGpu(0)
    yield g
    g.close()


# ------------------------------------------------------------------ normals
def check_normals(nrm, curv, pts, idx, k, viewpoint, what, coord_max=None, ref_pts=None):
    """GPU normals / curv of `pts` against ref_normals (of ref_pts when the
    GPU ran on a translated copy). Returns the share of points left out."""
    rp = pts if ref_pts is None else ref_pts
    vp = None if viewpoint is None else np.asarray(viewpoint) - (pts[0] - rp[0])
    rn, rc, valid, lam = ref_normals(rp, idx, k, vp)
    n = len(rp)
    gv = ~np.isnan(curv)
    assert np.array_equal(gv, valid), what                      # the split, exactly
    assert np.array_equal(nrm[~valid], np.zeros(((~valid).sum(), 3))), what
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = lam[:, 1] / lam[:, 2]
        assert not ((ratio >= 1e-14) & (ratio <= 1e-9)).any(), what
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        cmp = valid & (gap >= 1e-6)
        cm = np.abs(pts).max() if coord_max is None else coord_max
        scale = 1024 * EPS * (1.0 + cm / np.sqrt(lam[:, 2]))
        tol_n = scale / gap
    left_out = 1.0 - cmp.sum() / n
    if not cmp.any():
        return left_out
    g, r, tol = nrm[cmp], rn[cmp], tol_n[cmp]
    # where the orientation rule itself sits within the tolerance of its
    # threshold, either sign is right
    if vp is None:
        a = np.sort(np.abs(r), axis=1)
        amb = a[:, 2] - a[:, 1] <= 2 * tol
    else:
        d = vp.reshape(1, 3) - rp[cmp]
        amb = np.abs((r * d).sum(1)) <= tol * np.linalg.norm(d, axis=1)
    e_same = np.abs(g - r).max(1)
    e_flip = np.abs(g + r).max(1)
    err = np.where(amb, np.minimum(e_same, e_flip), e_same)
    ec = np.abs(curv[cmp] - rc[cmp])
    print(f"{what}: n {n} compared {cmp.sum()} invalid {(~valid).sum()} ambiguous {amb.sum()} "
          f"max err/tol normal {np.max(err / tol):.3g} curv {np.max(ec / scale[cmp]):.3g}")
    assert (err <= tol).all(), what
    assert (ec <= scale[cmp]).all(), what
    assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() <= 16 * EPS, what
    return left_out


def rows(idx, stride):
    """idx rows widened to `stride` slots, the unused ones filled with -5"""
    out = np.full((len(idx), stride), -5, np.int32)
    out[:, :idx.shape[1]] = idx
    return out


def normals_dev(gpu, pts, idx, k, viewpoint, alloc=None):
    """navgpu_normals_dev on device tensors; alloc: a larger cloud whose first
    len(pts) points are pts"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(pts)
    src = pts if alloc is None else alloc
    d_pts = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    d_n = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
    d_c = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gpu.normals_dev(d_pts, n, d_idx, idx.shape[1], k, viewpoint, d_n, d_c)
    gpu.sync()
    return d_n.cpu().numpy(), d_c.cpu().numpy()


VIEW = (400.0, -2500.0, 900.0)


@pytest.mark.parametrize("k,stride", [(3, 3), (8, 8), (8, 16), (16, 16)])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 4097])
def test_normals_match_restatement(gpu, n, k, stride):
    rng = np.random.default_rng(1000 * n + k)
    pts = rng.uniform(0.0, 1000.0, (n, 3))
    kk = min(k, n)
    nn = np.full((n, k), -1, np.int32)
    nn[:, :kk] = knn_numpy(pts, pts, kk)[0]
    idx = rows(nn, stride)
    for vp in (None, VIEW):
        nrm, curv = normals_dev(gpu, pts, idx, k, vp)
        out = check_normals(nrm, curv, pts, idx, k, vp, f"n={n} k={k} stride={stride} vp={vp}")
        assert out <= 0.02 or n < 3


def test_normals_second_trip(gpu):
    n = NORM_ONE_TRIP + 1
    rng = np.random.default_rng(2)
    pts = rng.uniform(0.0, 1000.0, (n, 3))
    idx = rng.integers(0, n, (n, 3)).astype(np.int32)
    nrm, curv = normals_dev(gpu, pts, idx, 3, VIEW)
    assert check_normals(nrm, curv, pts, idx, 3, VIEW, "second trip") <= 0.02


def test_normals_room_cloud(gpu):
    # the dropout points are zero-filled and coincide: invalid by rule
    _, tgt = l9_clouds()
    idx, _ = knn_numpy(tgt, tgt, 8)
    nrm, curv = normals_dev(gpu, tgt, idx, 8, (0.0, 0.0, 0.0))
    out = check_normals(nrm, curv, tgt, idx, 8, (0.0, 0.0, 0.0), "room")
    assert 0 < np.isnan(curv).sum() and out <= 0.02


def test_normals_degenerate_rows(gpu):
    rng = np.random.default_rng(4)
    n, k = 64, 8
    alloc = rng.uniform(0.0, 1000.0, (n + 16, 3))   # a stray read lands in owned memory
    pts = alloc[:n]
    pts[8:16] = pts[8]                              # k coincident points
    pts[16:24] = np.outer(np.arange(8.0), [3.0, -2.0, 5.0]) + np.array([10.0, 20.0, -30.0])
    idx = rng.integers(24, n, (n, k)).astype(np.int32)
    idx[0, 2:] = -1                                 # 2 valid slots
    idx[1] = -1
    idx[2] = [n, n + 5, -7, n, n + 5, -7, n, n + 5]
    idx[3] = np.arange(8, 16)                       # coincident
    idx[4] = np.arange(16, 24)                      # integer collinear
    idx[5] = [-1, 30, -7, 31, n, 32, n + 5, -1]     # exactly 3 valid, not collinear
    bad = [0, 1, 2, 3, 4]
    for vp in (None, VIEW):
        nrm, curv = normals_dev(gpu, pts, idx, k, vp, alloc=alloc)
        assert np.array_equal(nrm[bad], np.zeros((5, 3))) and np.isnan(curv[bad]).all()
        check_normals(nrm, curv, pts, idx, k, vp, f"degenerate vp={vp}")
        # the triangle's normal
        tri = np.cross(pts[31] - pts[30], pts[32] - pts[30])
        tri /= np.linalg.norm(tri)
        assert np.abs(np.abs(nrm[5] @ tri) - 1.0) <= 1e-9 and curv[5] <= 1e-12
        ok = ~np.isnan(curv)
        assert ok.sum() == n - 5
        if vp is None:
            big = np.argmax(np.abs(nrm[ok]), axis=1)
            assert (nrm[ok][np.arange(ok.sum()), big] > 0).all()
        else:
            d = np.asarray(vp) - pts[ok]
            assert ((nrm[ok] * d).sum(1) >= -1024 * EPS * np.linalg.norm(d, axis=1)).all()


def test_normals_large_offset_and_far_side(gpu):
    rng = np.random.default_rng(6)
    n = 4096
    flat = np.column_stack([rng.uniform(0.0, 1000.0, n), rng.uniform(0.0, 1000.0, n),
                            rng.normal(0.0, 1.0, n)]) @ rot((1, 2, 3), 35.0).T
    flat = np.round(flat * 1024.0) / 1024.0         # the offset then adds exactly
    off = np.array([1e7, -1e7, 1e7])
    far = flat + off
    assert np.array_equal(far - off, flat)
    idx, _ = knn_numpy(flat, flat, 8)
    vp = (0.0, 0.0, 5000.0)
    n0, c0 = normals_dev(gpu, flat, idx, 8, vp)
    assert check_normals(n0, c0, flat, idx, 8, vp, "offset 0") <= 0.02
    n1, c1 = normals_dev(gpu, far, idx, 8, tuple(np.asarray(vp) + off))
    out = check_normals(n1, c1, far, idx, 8, tuple(np.asarray(vp) + off), "offset 1e7",
                        coord_max=np.abs(far).max(), ref_pts=flat)
    assert out <= 0.02
    # viewpoints 5 m off the patch on either side of it: every normal flips,
    # and nothing else changes
    up = rot((1, 2, 3), 35.0) @ np.array([0.0, 0.0, 5000.0])
    n_up, _ = normals_dev(gpu, flat, idx, 8, tuple(flat.mean(0) + up))
    n_dn, _ = normals_dev(gpu, flat, idx, 8, tuple(flat.mean(0) - up))
    assert (~np.isnan(c0)).all() and (n_up @ up > 0).all()
    assert np.array_equal(n_dn, -n_up)


def test_cloud_normals_equals_two_calls(gpu):
    _, tgt = l9_clouds()
    a_n, a_c = gpu.normals(tgt, k=8)
    idx, _ = gpu.knn(tgt, tgt, 8)
    b_n, b_c = gpu.normals(tgt, k=8, idx=idx)
    assert a_n.tobytes() == b_n.tobytes() and a_c.tobytes() == b_c.tobytes()
    assert (~np.isnan(a_c)).sum() >= 4000
    v_n, v_c = gpu.normals(tgt, k=8, viewpoint=(0.0, 0.0, 0.0))
    w_n, w_c = gpu.normals(tgt, k=8, viewpoint=(0.0, 0.0, 0.0), idx=idx)
    assert v_n.tobytes() == w_n.tobytes() and v_c.tobytes() == w_c.tobytes()
    # and the device-pointer entry point
    import torch
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(np.ascontiguousarray(tgt)).to(dev)
    d_n = torch.zeros((len(tgt), 3), dtype=torch.float64, device=dev)
    d_c = torch.zeros(len(tgt), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gpu.cloud_normals_dev(d_pts, len(tgt), 8, (0.0, 0.0, 0.0), d_n, d_c)
    gpu.sync()
    gpu.knn_check()
    assert d_n.cpu().numpy().tobytes() == v_n.tobytes()
    assert d_c.cpu().numpy().tobytes() == v_c.tobytes()


# --------------------------------------------------------------- plane step
R_TRUE = rot((1, -2, 3), 0.4)
T_TRUE = np.array([3.0, -2.0, 1.5])


def box_pose(nq, seed):
    """p ~ U[0,1000)^3, its image under a small motion stored in shuffled
    order as the target, one axis normal (either sign) and a curvature per
    target point, and the k-NN-shaped idx / dist that pair them"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1000.0, (nq, 3))
    q = p @ R_TRUE.T + T_TRUE
    perm = rng.permutation(nq).astype(np.int32)
    tgt = np.empty_like(q)
    tgt[perm] = q
    # every axis as often as the others, so that six pairs already give rank 6
    nrm = np.eye(3)[rng.permutation(nq) % 3] * rng.choice([-1.0, 1.0], nq)[:, None]
    curv = rng.uniform(0.0, 0.1, nq)
    dist = np.sqrt(((tgt[perm] - p) ** 2).sum(1))
    return p, tgt, nrm, curv, perm, dist


@pytest.mark.parametrize("stride", [1, 8])
@pytest.mark.parametrize("nq", [5, 6, 64, 65, 4097, PLANE_ONE_TRIP + 1])
def test_plane_known_pose(gpu, nq, stride):
    p, tgt, nrm, curv, idx, dist = box_pose(nq, seed=nq)
    I, D = strided(idx, dist, stride)
    R, t, stats = gpu.align_plane(p, tgt, nrm, curv, I, D)
    if nq < 6:
        assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
        r = ((tgt[idx] - p) * nrm[idx]).sum(1)
        before = np.sqrt((r ** 2).sum() / nq)
        assert stats[0] == nq and stats[3] == 0 and stats[4] == 0 and stats[5] == 0
        assert abs(stats[1] - before) <= 1024 * EPS * before and stats[2] == stats[1]
        return
    ref = ref_plane(p, tgt[idx], nrm[idx])
    assert ref["pivots"].min() >= 1e-6          # solved, and far from the refusal threshold
    assert stats[3] == 0
    check_step(R, t, stats, ref, what=f"nq={nq} stride={stride}")
    if nq >= 64:
        assert ref["kappa"] <= 1e3
        assert np.abs(R - R_TRUE).max() <= 1e-3 and np.abs(t - T_TRUE).max() <= 0.5


def test_plane_empty_call_and_equal_normals(gpu):
    z3 = np.zeros((0, 3))
    R, t, stats = gpu.align_plane(z3, np.zeros((5, 3)), np.zeros((5, 3)), np.zeros(5),
                                  np.zeros((0, 1), np.int32), np.zeros((0, 1)))
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert np.array_equal(stats, np.zeros(6))
    p, tgt, nrm, curv, idx, dist = box_pose(500, seed=12)
    for normal in ((0.0, 0.0, 1.0), (1.0 / 3, 2.0 / 3, 2.0 / 3)):
        same = np.tile(np.asarray(normal), (500, 1))
        R, t, stats = gpu.align_plane(p, tgt, same, curv, idx, dist)
        assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
        assert stats[0] == 500 and stats[4] == 0 and stats[2] == stats[1] and stats[5] <= 1e-10
    with pytest.raises(Exception):
        gpu.align_plane(p, tgt, nrm, curv, idx, dist, max_dist=np.nan)
    with pytest.raises(Exception):
        gpu.align_plane(p, tgt, nrm, curv, idx, dist, max_curv=np.nan)


def test_plane_gating(gpu):
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 4096
    rng = np.random.default_rng(33)
    p = rng.uniform(0.0, 1000.0, (nq, 3))
    q = p @ R_TRUE.T + T_TRUE + rng.normal(0.0, 0.5, (nq, 3))
    perm = rng.permutation(nq).astype(np.int32)
    alloc = rng.uniform(0.0, 1000.0, (nt + 16, 3))  # a stray index lands in owned memory
    alloc[perm] = q
    nalloc = np.eye(3)[rng.integers(0, 3, nt + 16)]
    calloc = rng.uniform(0.0, 0.1, nt + 16)
    idx = perm.copy()
    dist = np.sqrt(((alloc[idx] - p) ** 2).sum(1))
    max_dist = np.sort(dist)[-301]                  # the 300 largest fail the gate
    max_curv = 0.09                                 # about a tenth of the curvatures fail
    mask = np.ones(nq, np.int32)
    cls = rng.permutation(nq)
    none, past, past5, neg7, nan, mz, cnan = (cls[0:100], cls[100:150], cls[150:200],
                                              cls[200:260], cls[260:340], cls[340:740],
                                              cls[740:800])
    idx[none] = -1
    idx[past] = nt
    idx[past5] = nt + 5
    idx[neg7] = -7
    dist[nan] = np.nan
    mask[mz] = 0
    calloc[perm[cnan]] = np.nan                     # no normal at the neighbour
    with np.errstate(invalid="ignore"):
        gate = dist <= max_dist
    inr = (idx >= 0) & (idx < nt)
    cv = calloc[np.where(inr, idx, 0)]
    with np.errstate(invalid="ignore"):
        cgate = cv <= max_curv
    # every rejection class is present, and alone somewhere
    assert (idx == -1).sum() == 100 and (idx == nt).sum() == 50 and (idx == nt + 5).sum() == 50
    assert (idx == -7).sum() == 60 and np.isnan(dist).sum() == 80 and (mask == 0).sum() == 400
    others = inr & (mask != 0) & gate
    assert (inr & (mask != 0) & ~gate & ~np.isnan(dist) & cgate).sum() > 0
    assert (inr & (mask != 0) & np.isnan(dist) & cgate).sum() > 0
    assert (inr & gate & (mask == 0) & cgate).sum() > 0
    assert (others & np.isnan(cv)).sum() > 0
    assert (others & ~np.isnan(cv) & ~cgate).sum() > 0
    keep = others & cgate
    n_bad = int(((idx < -1) | (idx >= nt)).sum())
    assert keep.sum() >= 1000 and n_bad == 160
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_src, d_tgt, d_idx, d_dist, d_mask = to(p), to(alloc), to(idx), to(dist), to(mask)
    d_n, d_c = to(nalloc), to(calloc)
    out = torch.zeros(18, dtype=torch.float64, device=dev)
    P0 = np.concatenate([rot((0, 0, 1), 10.0).ravel(), [1.0, 2.0, 3.0]])
    pose = to(P0)
    torch.cuda.synchronize()
    gpu.align_plane_dev(d_src, nq, d_tgt, nt, d_n, d_c, d_idx, d_dist, 1, max_dist, max_curv,
                        d_mask, out, pose, out[12:])
    gpu.sync()
    o = out.cpu().numpy()
    R, t, stats = o[:9].reshape(3, 3), o[9:12], o[12:]
    assert stats[0] == keep.sum() and stats[3] == n_bad
    ref = ref_plane(p[keep], alloc[idx[keep]], nalloc[idx[keep]])
    assert ref["kappa"] <= 1e3
    check_step(R, t, stats, ref, what="gating")
    # pose <- delta o pose, in pose_compose's operation order
    want = np.empty(12)
    for i in range(3):
        a, b, c = o[3 * i], o[3 * i + 1], o[3 * i + 2]
        for j in range(3):
            want[3 * i + j] = (a * P0[j] + b * P0[3 + j]) + c * P0[6 + j]
        want[9 + i] = ((a * P0[9] + b * P0[10]) + c * P0[11]) + o[9 + i]
    assert np.array_equal(pose.cpu().numpy(), want)


def test_plane_deterministic():
    from navslam.gpu import NavGpu
    nq = 70001
    p, tgt, _, _, idx, dist = box_pose(nq, seed=5)
    rng = np.random.default_rng(6)
    tgt = tgt + rng.normal(0.0, 2.0, tgt.shape)
    mask = (rng.random(nq) < 0.8).astype(np.int32)
    runs = []

    def once(g):
        ki, _ = g.knn(tgt, tgt, 8)
        nrm, curv = g.normals(tgt, k=8, viewpoint=(0.0, 0.0, 0.0), idx=ki)
        ok = ~np.isnan(curv)
        R, t, stats = g.align_plane(p, tgt, nrm, curv, idx, dist, max_dist=np.median(dist),
                                    max_curv=np.median(curv[ok]), mask=mask)
        return nrm, curv, R, t, stats

    g = NavGpu(0)
    runs.append(once(g))
    runs.append(once(g))
    g.close()
    g = NavGpu(0)
    runs.append(once(g))
    g.close()
    assert 6 <= runs[0][4][0] < nq and runs[0][4][4] == 1
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------- ICP
def test_icp_plane_steps_match_restatement(gpu, orc):
    src, tgt = l9_clouds()
    gate, iters, vp = 150.0, 4, (0.0, 0.0, 0.0)
    nrm, curv = gpu.normals(tgt, k=8, viewpoint=vp)
    valid = ~np.isnan(curv)
    R, t, stats, hist = gpu.icp_plane(src, tgt, nrm, curv, iters=iters, max_dist=gate)
    assert np.array_equal(hist[-1], np.concatenate([R.ravel(), t]))
    # the host entry point that computes the normals itself: byte for byte
    R2, t2, stats2, hist2 = gpu.icp_plane(src, tgt, iters=iters, max_dist=gate, kn=8,
                                          viewpoint=vp)
    for a, b in ((R, R2), (t, t2), (stats, stats2), (hist, hist2)):
        assert a.tobytes() == b.tobytes()
    # and the device-pointer entry point
    import torch
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_pose = to(np.concatenate([np.eye(3).ravel(), np.zeros(3)]))
    d_hist = torch.zeros((iters, 12), dtype=torch.float64, device=dev)
    d_stats = torch.zeros((iters, 6), dtype=torch.float64, device=dev)
    d_src, d_tgt, d_nrm, d_curv = to(src), to(tgt), to(nrm), to(curv)
    torch.cuda.synchronize()
    gpu.icp_plane_dev(d_src, len(src), d_tgt, len(tgt), d_nrm, d_curv, iters, gate, np.inf,
                      None, d_pose, d_hist, d_stats)
    gpu.sync()
    assert d_hist.cpu().numpy().tobytes() == hist.tobytes()
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes()
    assert np.array_equal(d_pose.cpu().numpy(), hist[-1])
    prev = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    for i in range(iters):
        cur = apply_pose(prev, src)
        idx, dist = orc.knn_brute(tgt, cur, 1)
        idx, dist = idx[:, 0], dist[:, 0]
        assert np.abs(dist - gate).min() > 1e-6      # no pair sits on the gate
        keep = (idx >= 0) & (dist <= gate) & valid[np.maximum(idx, 0)]
        assert keep.sum() >= 3000
        assert stats[i][0] == keep.sum(), i
        assert stats[i][3] == 0
        ref = ref_plane(cur[keep], tgt[idx[keep]], nrm[idx[keep]])
        assert ref["kappa"] <= 1e3
        want_R = ref["R"] @ prev[:9].reshape(3, 3)
        want_t = ref["R"] @ prev[9:] + ref["t"]
        # the composition carries the step's error: |dR| for R, and for t
        # |dR| |t_prev| + |dt|
        tol_R = 3 * ref["tol_R"] + 16 * EPS
        tol_t = 3 * ref["tol_R"] * np.linalg.norm(prev[9:]) + ref["tol_t"] \
            + 64 * EPS * np.abs(want_t).max()
        eR = np.abs(hist[i][:9].reshape(3, 3) - want_R).max()
        et = np.abs(hist[i][9:] - want_t).max()
        print(f"icp_plane {i}: kept {keep.sum()} kappa {ref['kappa']:.3g} |dR| {eR:.3g} "
              f"(tol {tol_R:.3g}) |dt| {et:.3g} (tol {tol_t:.3g}) rms {stats[i][1]:.4g} -> "
              f"{stats[i][2]:.4g} min pivot {stats[i][5]:.3g}")
        assert eR <= tol_R and et <= tol_t, i
        assert stats[i][4] == 1
        assert abs(stats[i][1] - ref["before"]) <= 1024 * EPS * ref["before"]
        prev = hist[i]


def pose_errors(hist):
    """translation (mm) and rotation (degrees) error of each pose against the
    true motion of l9_pair's default step"""
    Rt = rot((0, 0, 1), 0.8).T
    tt = -Rt @ np.array([120.0, -40.0, 5.0])
    et, er = [], []
    for h in hist:
        Rm = h[:9].reshape(3, 3)
        et.append(np.linalg.norm(h[9:] - tt))
        c = (np.trace(Rm @ Rt.T) - 1.0) / 2.0
        er.append(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    return np.array(et), np.array(er)


def test_icp_plane_beats_point_to_point_on_the_room(gpu):
    src, tgt = l9_clouds()
    gate = 150.0
    _, _, _, h_pl = gpu.icp_plane(src, tgt, iters=3, max_dist=gate, kn=8,
                                  viewpoint=(0.0, 0.0, 0.0))
    _, _, _, h_pt = gpu.icp(src, tgt, iters=6, max_dist=gate)
    t_pl, r_pl = pose_errors(h_pl)
    t_pt, r_pt = pose_errors(h_pt)
    print("point-to-plane  mm:", np.array2string(t_pl, precision=3), "deg:",
          np.array2string(r_pl, precision=4))
    print("point-to-point  mm:", np.array2string(t_pt, precision=3), "deg:",
          np.array2string(r_pt, precision=4))
    assert t_pl[-1] <= 0.5 * t_pt[-1]
    assert r_pl[-1] <= 0.5 * r_pt[-1]
