"""sha256 of every output array of the registration on seeded inputs: the
check that a change to align.hip, plane.hip or their shared headers leaves the
results as they were, to the bit. GPU only.

The sums are reproducible by construction (DESIGN.md §10 "Determinism"), so
two builds of the library that compute the same thing print the same digests.
Run it once per build, in separate processes (NAVGPU_LIB selects the library),
and compare the two JSON files: any difference is a changed result.

Per size nq in 4,097, 1,048,576 and one trip of the grid plus one for each
metric (1,048,577 point-to-point, 524,289 point-to-plane), and per variant
(plain; with a mask; with a mask and finite max_dist and max_curv) it runs
normals_dev with k = 8 (once per size), align_dev, align_plane_dev, and 5
iterations of icp_dev and icp_plane_dev. Writes the JSON to --out and prints
it on one line."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nav-slam_amd"))
from navslam.gpu import NavGpu  # noqa: E402

SIZES = (4097, 1 << 20, 1024 * 256 * 4 + 1, 1024 * 256 * 2 + 1)
ITERS = 5
KN = 8


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def clouds(n):
    """a uniform cloud at the density of 1,048,576 points in a 1 m cube, and
    its image under a small motion plus noise, in shuffled order"""
    rng = np.random.default_rng(n)
    side = 1000.0 * (n / float(1 << 20)) ** (1.0 / 3.0)
    src = rng.uniform(0.0, side, (n, 3))
    c, s = np.cos(np.deg2rad(0.4)), np.sin(np.deg2rad(0.4))
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tgt = (src @ Rz.T + np.array([3.0, -2.0, 1.5]) + rng.normal(0.0, 1.0, (n, 3)))
    tgt = tgt[rng.permutation(n)]
    mask = (rng.random(n) < 0.8).astype(np.int32)
    return src, tgt, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    g = NavGpu(0)
    f64 = dict(dtype=torch.float64, device=dev)
    res = {}
    for n in SIZES:
        s, t, m = clouds(n)
        src, tgt, mask = (torch.from_numpy(x).to(dev) for x in (s, t, m))
        idx8 = torch.zeros((n, KN), dtype=torch.int32, device=dev)
        dist8 = torch.zeros((n, KN), **f64)
        idx1 = torch.zeros((n, 1), dtype=torch.int32, device=dev)
        dist1 = torch.zeros((n, 1), **f64)
        nrm, curv = torch.zeros((n, 3), **f64), torch.zeros(n, **f64)
        torch.cuda.synchronize()
        g.knn_dev(tgt, n, tgt, n, KN, idx8, dist8)
        g.normals_dev(tgt, n, idx8, KN, KN, (0.0, 0.0, 0.0), nrm, curv)
        g.knn_dev(tgt, n, src, n, 1, idx1, dist1)
        g.sync()
        g.knn_check()
        out = {"normals": sha(nrm), "curv": sha(curv)}
        gate = float(np.median(dist1.cpu().numpy()))
        cgate = float(np.nanmedian(curv.cpu().numpy()))
        for name, mk, md, mc in (("plain", None, np.inf, np.inf), ("mask", mask, np.inf, np.inf),
                                 ("mask_gates", mask, gate, cgate)):
            o16, o18 = torch.zeros(16, **f64), torch.zeros(18, **f64)
            pose0 = torch.from_numpy(np.concatenate([np.eye(3).ravel(), np.zeros(3)])).to(dev)
            p_a, p_p, p_i, p_ip = (pose0.clone() for _ in range(4))
            h_i, h_ip = torch.zeros((ITERS, 12), **f64), torch.zeros((ITERS, 12), **f64)
            s_i, s_ip = torch.zeros((ITERS, 4), **f64), torch.zeros((ITERS, 6), **f64)
            torch.cuda.synchronize()
            g.align_dev(src, n, tgt, n, idx1, dist1, 1, md, mk, o16, p_a, o16[12:])
            g.align_plane_dev(src, n, tgt, n, nrm, curv, idx1, dist1, 1, md, mc, mk, o18, p_p,
                              o18[12:])
            g.icp_dev(src, n, tgt, n, ITERS, md, mk, p_i, h_i, s_i)
            g.icp_plane_dev(src, n, tgt, n, nrm, curv, ITERS, md, mc, mk, p_ip, h_ip, s_ip)
            g.sync()
            g.knn_check()
            out[name] = {"align": sha(o16), "align_pose": sha(p_a),
                         "align_plane": sha(o18), "align_plane_pose": sha(p_p),
                         "icp_pose": sha(p_i), "icp_hist": sha(h_i), "icp_stats": sha(s_i),
                         "icp_plane_pose": sha(p_ip), "icp_plane_hist": sha(h_ip),
                         "icp_plane_stats": sha(s_ip),
                         "pairs": [int(o16[12].item()), int(o18[12].item())],
                         "solved": int(o18[16].item())}
        res[f"nq_{n}"] = out
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
