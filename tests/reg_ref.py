"""numpy restatements of the registration, shared by
tests/test_align_solve.py and tests/test_plane_solve.py (CPU) and
tests/test_gpu_align.py, tests/test_gpu_plane.py and tests/test_gpu_icp_host.py:
the rigid fit by SVD, the normals of a cloud from given neighbour rows, the
centred 6 x 6 step and its tolerances, and the inputs the tests share. The
reference project has none of this, so these are the checkers.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LINE_TOL = 1e-12   # kPlaneLineTol
PIVOT_MIN = 1e-10  # kPlanePivotMin


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def ref_align(p, q):
    """Least-squares R, t with q ~ R p + t: f64 centroids, centred H, Kabsch
    by SVD with the determinant fix. Also the singular values s of H, the sign
    d and the 20 centred moments align_solve takes (align_solve.h):
    m[17] + m[18] is Spp + Sqq."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n = len(p)
    pb = p.mean(0) if n else np.zeros(3)
    qb = q.mean(0) if n else np.zeros(3)
    pc, qc = p - pb, q - qb
    H = pc.T @ qc
    U, s, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    t = qb - R @ pb
    m = np.concatenate([[n], pb, qb, [((q - p) ** 2).sum()], H.ravel(),
                        [(pc ** 2).sum(), (qc ** 2).sum()], [0.0]])
    return R, t, s, d, m


def apply_pose(pose, pts):
    """k_transform's operation order: t + ((R0 x + R1 y) + R2 z)"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    for i in range(3):
        out[:, i] = pose[9 + i] + ((pose[3 * i] * x + pose[3 * i + 1] * y) + pose[3 * i + 2] * z)
    return out


def strided(idx, dist, stride):
    """rows of `stride` slots whose slot 0 is idx / dist and whose other slots
    would break the fit if they were read"""
    I = np.full((len(idx), stride), -5, np.int32)
    D = np.full((len(idx), stride), np.nan)
    I[:, 0] = idx
    D[:, 0] = dist
    return I, D


_L9 = {}


def l9_clouds():
    """l9_pair(16, 256, seed=3) as two clouds of 4,096 points, made once"""
    if not _L9:
        from navslam.synth import l9_pair
        src, tgt = l9_pair(16, 256, seed=3)
        _L9["pair"] = (src.reshape(-1, 3), tgt.reshape(-1, 3))
    return _L9["pair"]


def ref_normals(pts, idx, k, viewpoint=None):
    """normals[n,3], curv[n], valid[n], lam[n,3] (ascending, of the centred
    covariance of the valid slots among the first k of each idx row), by
    numpy.linalg.eigh, with the kernel's validity and orientation rules."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    idx = np.asarray(idx)[:, :k].astype(np.int64)
    ok = (idx >= 0) & (idx < n)
    x = pts[np.where(ok, idx, 0)]                       # [n, k, 3]
    w = ok[:, :, None].astype(np.float64)
    m = ok.sum(1)
    mu = (x * w).sum(1) / np.maximum(m, 1)[:, None]
    xc = (x - mu[:, None, :]) * w
    C = np.einsum("nki,nkj->nij", xc, xc)
    lam, vec = np.linalg.eigh(C)
    nrm = vec[:, :, 0].copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        valid = (m >= 3) & (lam[:, 2] > 0) & (lam[:, 1] > LINE_TOL * lam[:, 2])
        curv = np.maximum(lam[:, 0], 0.0) / lam.sum(1)
    if viewpoint is not None:
        d = np.asarray(viewpoint, np.float64).reshape(1, 3) - pts
        flip = (nrm * d).sum(1) < 0
    else:
        big = np.argmax(np.abs(nrm), axis=1)            # lowest index on ties
        flip = nrm[np.arange(n), big] < 0
    nrm[flip] *= -1.0
    nrm[~valid] = 0.0
    curv = np.where(valid, curv, np.nan)
    return nrm, curv, valid, lam


def plane_system(p, q, nrm):
    """pbar, J (rows [x cross n, n], x = p - pbar) and r = (q - p) . n"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float64).reshape(-1, 3)
    pb = p.mean(0) if len(p) else np.zeros(3)
    J = np.concatenate([np.cross(p - pb, nrm), nrm], axis=1)
    r = ((q - p) * nrm).sum(1)
    return pb, J, r


def plane_moments(p, q, nrm, bad=0.0):
    """the 33 reduced moments plane_solve takes (plane_solve.h)"""
    pb, J, r = plane_system(p, q, nrm)
    A = J.T @ J
    return np.concatenate([[len(r)], pb, [bad], A[np.triu_indices(6)], J.T @ r, [(r * r).sum()]])


def cayley(om):
    """the rotation of the unit quaternion of (1, om / 2)"""
    w, x, y, z = np.concatenate([[1.0], 0.5 * np.asarray(om)]) / np.sqrt(1.0 + 0.25 * (om @ om))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def ref_plane(p, q, nrm):
    """The step by numpy: a dict with R, t, x = (omega, tau), the diagonal D
    of A, kappa = cond_2 of S = D^-1/2 A D^-1/2, sum r^2, the rms before and
    the linear model's rms after, and the tolerances tol_y (on D^1/2 (x -
    x_ref), 2-norm), tol_R and tol_t (max-norm), for data of magnitude
    coord_max.

    tol_y = 1024 eps kappa (|D^1/2 x| + sqrt(sum r^2)): the relative error of
    the summed S and of the factorisation moves y = D^1/2 x by eps kappa |y|,
    the error of the summed right-hand side D^-1/2 b, at most eps sqrt(sum r^2)
    per unit column, by eps kappa sqrt(sum r^2); 1024 covers the <= 20-level
    summation tree, the 6 x 6 factorisation and the reference's own solve.
    |d omega_i| <= tol_y / sqrt(D_ii) and the Cayley map is a contraction
    (d angle / d |omega| <= 1), so tol_R = |d omega| + 16 eps (the rounding
    of the nine entries). t = tau + pbar - R pbar gives tol_t = |d tau| +
    2 tol_R |pbar| + 64 eps coord_max."""
    pb, J, r = plane_system(p, q, nrm)
    A, b = J.T @ J, J.T @ r
    D = np.diag(A).copy()
    sd = np.sqrt(D)
    S = A / np.outer(sd, sd)
    y = np.linalg.solve(S, b / sd)
    x = y / sd
    kappa = np.linalg.cond(S)
    Srr = (r * r).sum()
    R = cayley(x[:3])
    t = x[3:] + pb - R @ pb
    tol_y = 1024 * EPS * kappa * (np.linalg.norm(y) + np.sqrt(Srr))
    tol_R = np.sqrt((tol_y ** 2 / D[:3]).sum()) + 16 * EPS
    coord_max = max(np.abs(p).max(), np.abs(q).max())
    tol_t = np.sqrt((tol_y ** 2 / D[3:]).sum()) + 2 * tol_R * np.linalg.norm(pb) \
        + 64 * EPS * coord_max
    n = len(r)
    return dict(R=R, t=t, x=x, y=y, D=D, kappa=kappa, Srr=Srr, pb=pb, n=n,
                before=np.sqrt(Srr / n), after=np.sqrt(max(0.0, Srr - b @ x) / n),
                tol_y=tol_y, tol_R=tol_R, tol_t=tol_t, pivots=ldl_pivots(S))


def ldl_pivots(S):
    """pivots of the LDL^T factorisation of S without pivoting"""
    S = np.array(S, np.float64)
    L, d = np.eye(6), np.zeros(6)
    for j in range(6):
        d[j] = S[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
        for i in range(j + 1, 6):
            L[i, j] = (S[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / d[j]
    return d


def check_step(R, t, stats, ref, what=""):
    """delta = (R, t) and stats[6] of a solved step against ref_plane's dict"""
    eR, et = np.abs(R - ref["R"]).max(), np.abs(t - ref["t"]).max()
    print(f"{what}: n {ref['n']} kappa {ref['kappa']:.3g} |dR| {eR:.3g} (tol {ref['tol_R']:.3g}) "
          f"|dt| {et:.3g} (tol {ref['tol_t']:.3g}) rms {stats[1]:.6g} -> {stats[2]:.6g} "
          f"(ref {ref['after']:.6g}) min pivot {stats[5]:.4g}")
    assert stats[0] == ref["n"], what
    assert stats[4] == 1.0, what
    assert eR <= ref["tol_R"], what
    assert et <= ref["tol_t"], what
    assert abs(stats[1] - ref["before"]) <= 1024 * EPS * ref["before"], what
    # sum r^2 - b.x = sum r^2 - y.(D^-1/2 b): the error of y times |D^-1/2 b|
    # <= sqrt(6 sum r^2) (six unit columns), plus the rounding of sum r^2
    tol_res = ref["tol_y"] * np.sqrt(6 * ref["Srr"]) + 1024 * EPS * ref["Srr"]
    assert abs(stats[2] ** 2 - ref["after"] ** 2) * ref["n"] <= tol_res, what
    assert abs(stats[5] - ref["pivots"].min()) <= 1024 * EPS * ref["kappa"], what
    assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * EPS, what
    assert np.linalg.det(R) > 0, what


def knn_numpy(tgt, q, k):
    """brute-force k-NN ordered by (distance, index): idx[nq,k], dist[nq,k]"""
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    idx = np.empty((len(q), k), np.int32)
    dist = np.empty((len(q), k))
    for a in range(0, len(q), 512):
        d = tgt[None, :, :] - q[a:a + 512, None, :]
        d = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[a:a + 512] = o
        dist[a:a + 512] = np.take_along_axis(d, o, 1)
    return idx, dist
