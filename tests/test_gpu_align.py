"""The 6-DOF align step and the ICP loop on the GPU (align.hip) against the
numpy restatement ref_align of tests/reg_ref.py (Kabsch by SVD). The
reference project fits no rotation, so the restatement is the checker.

Tolerances come from the data: tol_R = 1024 eps kappa with kappa = s0 /
(s1 + d s2) the conditioning of the rotation (1024 covers the <= 20-level
summation tree and the Jacobi sweeps), tol_t = (2 tol_R + 64 eps) max|coord|,
and the rms after the step to sqrt(1024 eps (Spp + Sqq) / n) absolute. The
rms before the step is one sum of n non-negative terms: 1024 eps relative.
"""
import numpy as np
import pytest

from reg_ref import EPS, apply_pose, l9_clouds, ref_align, rot, strided

pytestmark = pytest.mark.gpu

# the moments kernel: at most 1024 blocks of 256 threads, each thread taking 4
# queries per trip of the grid-stride loop, so one trip of the whole launch
# covers 1024 * 256 * 4 queries; one more makes a second trip
ONE_TRIP = 1024 * 256 * 4


@pytest.fixture(scope="module")
def gpu():
    from navslam.gpu import NavGpu
    g = NavGpu(0)
    yield g
    g.close()


R0 = rot((1, 2, 3), 25.0)
T0 = np.array([120.0, -40.0, 5.0])


def check_fit(R, t, stats, p, q, n_bad=0, what=""):
    """R, t, stats of an align step against ref_align on the accepted pairs."""
    n = len(p)
    assert stats[0] == n, what
    assert stats[3] == n_bad, what
    Rr, tr, s, d, m = ref_align(p, q)
    S = m[17] + m[18]
    kappa = s[0] / (s[1] + d * s[2])
    tol_R = 1024 * EPS * kappa
    tol_t = (2 * tol_R + 64 * EPS) * max(np.abs(p).max(), np.abs(q).max())
    before = np.sqrt(((q - p) ** 2).sum() / n)
    after = np.sqrt((((p @ Rr.T + tr) - q) ** 2).sum() / n)
    eR, et = np.abs(R - Rr).max(), np.abs(t - tr).max()
    print(f"{what}: n {n} kappa {kappa:.3g} |dR| {eR:.3g} (tol {tol_R:.3g}) |dt| {et:.3g} "
          f"(tol {tol_t:.3g}) rms {stats[1]:.6g} -> {stats[2]:.3g} (ref {after:.3g})")
    assert eR <= tol_R, what
    assert et <= tol_t, what
    assert abs(stats[1] - before) <= 1024 * EPS * before, what
    assert abs(stats[2] - after) <= np.sqrt(1024 * EPS * S / n), what


def known_pose(nq, seed, offset=0.0):
    """p ~ U[0,1000)^3 (+ offset), its image under (R0, T0) stored in shuffled
    order as the target, and the k-NN-shaped idx / dist that pair them."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1000.0, (nq, 3))
    q = p @ R0.T + T0 + offset
    p = p + offset
    perm = rng.permutation(nq).astype(np.int32)
    tgt = np.empty_like(q)
    tgt[perm] = q
    dist = np.sqrt(((tgt[perm] - p) ** 2).sum(1))
    return p, tgt, perm, dist


@pytest.mark.parametrize("stride", [1, 8])
@pytest.mark.parametrize("nq", [1, 2, 3, 63, 64, 65, 255, 257, 4097, ONE_TRIP + 1])
def test_align_known_pose(gpu, nq, stride):
    p, tgt, idx, dist = known_pose(nq, seed=nq)
    I, D = strided(idx, dist, stride)
    R, t, stats = gpu.align(p, tgt, I, D)
    if nq < 3:
        assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
        before = np.sqrt((dist ** 2).sum() / nq)
        assert stats[0] == nq and stats[3] == 0
        assert abs(stats[1] - before) <= 1024 * EPS * before and stats[2] == stats[1]
        return
    check_fit(R, t, stats, p, tgt[idx], what=f"nq={nq} stride={stride}")


def test_align_empty_call_gives_identity(gpu):
    R, t, stats = gpu.align(np.zeros((0, 3)), np.zeros((5, 3)), np.zeros((0, 1), np.int32),
                            np.zeros((0, 1)))
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    assert np.array_equal(stats, np.zeros(4))


def test_align_large_offset(gpu):
    p, tgt, idx, dist = known_pose(4096, seed=21, offset=1e7)
    R, t, stats = gpu.align(p, tgt, idx, dist)
    check_fit(R, t, stats, p, tgt[idx], what="offset 1e7")


def test_align_gating(gpu):
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 4096
    rng = np.random.default_rng(33)
    p = rng.uniform(0.0, 1000.0, (nq, 3))
    q = p @ R0.T + T0 + rng.normal(0.0, 2.0, (nq, 3))
    perm = rng.permutation(nq).astype(np.int32)
    alloc = rng.uniform(0.0, 1000.0, (nt + 16, 3))  # a stray index lands in owned memory
    alloc[perm] = q
    idx = perm.copy()
    dist = np.sqrt(((alloc[idx] - p) ** 2).sum(1))
    max_dist = np.sort(dist)[-301]                  # the 300 largest fail the gate
    mask = np.ones(nq, np.int32)
    cls = rng.permutation(nq)
    none, past, past5, neg7, nan, mz = (cls[0:100], cls[100:150], cls[150:200], cls[200:260],
                                        cls[260:340], cls[340:740])
    idx[none] = -1
    idx[past] = nt
    idx[past5] = nt + 5
    idx[neg7] = -7
    dist[nan] = np.nan
    mask[mz] = 0
    with np.errstate(invalid="ignore"):
        gate = dist <= max_dist
    inr = (idx >= 0) & (idx < nt)
    # every rejection class is present, and alone somewhere
    assert (idx == -1).sum() == 100 and (idx == nt).sum() == 50 and (idx == nt + 5).sum() == 50
    assert (idx == -7).sum() == 60 and np.isnan(dist).sum() == 80 and (mask == 0).sum() == 400
    assert (inr & (mask != 0) & ~gate & ~np.isnan(dist)).sum() > 0
    assert (inr & (mask != 0) & np.isnan(dist)).sum() > 0
    assert (inr & gate & (mask == 0)).sum() > 0
    keep = inr & gate & (mask != 0)
    n_bad = int(((idx < -1) | (idx >= nt)).sum())
    assert keep.sum() >= 1000 and n_bad == 160
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_src, d_tgt, d_idx, d_dist, d_mask = to(p), to(alloc), to(idx), to(dist), to(mask)
    out = torch.zeros(16, dtype=torch.float64, device=dev)
    pose = to(np.concatenate([rot((0, 0, 1), 10.0).ravel(), [1.0, 2.0, 3.0]]))
    torch.cuda.synchronize()
    gpu.align_dev(d_src, nq, d_tgt, nt, d_idx, d_dist, 1, max_dist, d_mask, out, pose, out[12:])
    gpu.sync()
    o = out.cpu().numpy()
    R, t, stats = o[:9].reshape(3, 3), o[9:12], o[12:]
    check_fit(R, t, stats, p[keep], alloc[idx[keep]], n_bad=n_bad, what="gating")
    # pose <- delta o pose, in pose_compose's operation order
    P0 = np.concatenate([rot((0, 0, 1), 10.0).ravel(), [1.0, 2.0, 3.0]])
    want = np.empty(12)
    for i in range(3):
        a, b, c = o[3 * i], o[3 * i + 1], o[3 * i + 2]
        for j in range(3):
            want[3 * i + j] = (a * P0[j] + b * P0[3 + j]) + c * P0[6 + j]
        want[9 + i] = ((a * P0[9] + b * P0[10]) + c * P0[11]) + o[9 + i]
    assert np.array_equal(pose.cpu().numpy(), want)


def test_align_deterministic():
    from navslam.gpu import NavGpu
    nq = 70001
    p, tgt, idx, dist = known_pose(nq, seed=5)
    rng = np.random.default_rng(6)
    tgt = tgt + rng.normal(0.0, 2.0, tgt.shape)
    mask = (rng.random(nq) < 0.8).astype(np.int32)
    runs = []
    g = NavGpu(0)
    runs.append(g.align(p, tgt, idx, dist, max_dist=np.median(dist), mask=mask))
    runs.append(g.align(p, tgt, idx, dist, max_dist=np.median(dist), mask=mask))
    g.close()
    g = NavGpu(0)
    runs.append(g.align(p, tgt, idx, dist, max_dist=np.median(dist), mask=mask))
    g.close()
    assert 3 <= runs[0][2][0] < nq
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_transform_pose_bitexact(gpu, n):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    pts = torch.from_numpy(rng.uniform(-5000.0, 5000.0, (n, 3))).to(dev)
    Rm, t = rot(rng.normal(size=3), 77.0), rng.uniform(-1e3, 1e3, 3)
    pose = torch.from_numpy(np.concatenate([Rm.ravel(), t])).to(dev)
    a = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    b = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    gpu.transform_dev(pts, n, Rm, t, None, a)
    gpu.transform_pose_dev(pts, n, pose, b)
    gpu.sync()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.abs(a.cpu().numpy()).max() > 0


def test_icp_steps_match_restatement(gpu, orc):
    src, tgt = l9_clouds()
    gate, iters = 150.0, 8
    R, t, stats, hist = gpu.icp(src, tgt, iters=iters, max_dist=gate)
    assert np.array_equal(hist[-1], np.concatenate([R.ravel(), t]))
    prev = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    for i in range(iters):
        cur = apply_pose(prev, src)
        idx, dist = orc.knn_brute(tgt, cur, 1)
        idx, dist = idx[:, 0], dist[:, 0]
        assert np.abs(dist - gate).min() > 1e-6      # no pair sits on the gate
        keep = (idx >= 0) & (dist <= gate)
        assert keep.sum() >= 3000
        assert stats[i][0] == keep.sum(), i
        assert stats[i][3] == 0
        p, q = cur[keep], tgt[idx[keep]]
        dR, dt, s, d, _ = ref_align(p, q)
        want_R = dR @ prev[:9].reshape(3, 3)
        want_t = dR @ prev[9:] + dt
        tol_R = 1024 * EPS * s[0] / (s[1] + d * s[2])
        tol_t = (2 * tol_R + 64 * EPS) * max(np.abs(cur).max(), np.abs(tgt).max())
        eR = np.abs(hist[i][:9].reshape(3, 3) - want_R).max()
        et = np.abs(hist[i][9:] - want_t).max()
        print(f"icp {i}: kept {keep.sum()} |dR| {eR:.3g} (tol {tol_R:.3g}) |dt| {et:.3g} "
              f"(tol {tol_t:.3g}) rms {stats[i][1]:.4g} -> {stats[i][2]:.4g}")
        assert eR <= tol_R and et <= tol_t, i
        prev = hist[i]


def test_icp_reduces_residual(gpu):
    src, tgt = l9_clouds()
    R, t, stats, hist = gpu.icp(src, tgt, iters=12)
    print("icp rms before each step:", np.array2string(stats[:, 1], precision=4))
    assert stats[-1][1] < stats[0][1]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 64 * EPS
