"""Timing of the align step and the ICP loop. GPU only.

Input: uniform_pair() (1,048,576 points a side) and its global k-NN for
k = 1 and k = 8 (the align step reads slot 0 of each k-wide row). Reports,
as medians over the timed calls after warm-up:
  * the "align" region (pass A, finish, pass B, solve) per call, the bytes
    its model counts (per query and pass: 24 B src + 4 B idx + 8 B dist +
    a 24-B gather), the rate that gives, and that rate as a fraction of the
    navgpu_stream_copy_dev ceiling measured in the same run;
  * a 10-iteration icp_dev split into its regions (k-NN build and query,
    transform, align) and its wall time.
Writes the JSON to --out (default profiles/align/bench_align.json) and
prints it on one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nav-slam_amd"))
from navslam.gpu import NavGpu  # noqa: E402
from navslam.synth import uniform_pair  # noqa: E402

BYTES_PER_QUERY_PASS = 24 + 4 + 8 + 24
PASSES = 2


def med(v):
    return round(float(np.median(v)), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align", "bench_align.json"))
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--icp-runs", type=int, default=10)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--cols", type=int, default=2048)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    g = NavGpu(0)
    s, t = uniform_pair(a.rows, a.cols)
    n = a.rows * a.cols
    src = torch.from_numpy(s.reshape(-1, 3)).to(dev)
    tgt = torch.from_numpy(t.reshape(-1, 3)).to(dev)
    out16 = torch.zeros(16, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    res = {"points": n, "calls": a.calls, "warmup": a.warmup,
           "bytes_model_per_query_pass": BYTES_PER_QUERY_PASS, "passes": PASSES}

    # the measured HBM ceiling: a streaming device-to-device copy
    nb = 256 << 20
    ca = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    cb = torch.ones(nb // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    g.timing(True)
    g.timing_select("stream_copy")
    ts = []
    for i in range(a.warmup + 20):
        g.stream_copy_dev(ca, cb, nb)
        g.sync()
        ms, _ = g.timing_read("stream_copy")
        if i >= a.warmup:
            ts.append(ms)
    copy_gbs = 2 * nb / (np.median(ts) * 1e-3) / 1e9
    res["stream_copy"] = {"bytes_each_way": nb, "ms_med": med(ts), "GBps": round(copy_gbs, 1)}
    del ca, cb

    g.timing_select("align")
    for k in (1, 8):
        idx = torch.zeros((n, k), dtype=torch.int32, device=dev)
        dist = torch.zeros((n, k), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        g.knn_dev(tgt, n, src, n, k, idx, dist)
        g.sync()
        ts = []
        for i in range(a.warmup + a.calls):
            g.align_dev(src, n, tgt, n, idx, dist, k, np.inf, None, out16, None, out16[12:])
            g.sync()
            ms, cnt = g.timing_read("align")
            assert cnt == 1
            if i >= a.warmup:
                ts.append(ms)
        o = out16.cpu().numpy()
        model = PASSES * BYTES_PER_QUERY_PASS * n
        gbs = model / (np.median(ts) * 1e-3) / 1e9
        res[f"align_k{k}"] = {
            "ms_med": med(ts), "ms_min": round(float(np.min(ts)), 5),
            "ms_p90": round(float(np.percentile(ts, 90)), 5), "bytes_model": model,
            "GBps_model": round(gbs, 1), "fraction_of_stream_copy": round(gbs / copy_gbs, 4),
            "pairs": int(o[12]), "rms_before": float(o[13]), "rms_after": float(o[14])}
        del idx, dist

    # a 10-iteration ICP, every region timed
    g.timing_select(None)
    iters = 10
    regions = ("icp_transform", "knn_build", "knn_query", "align")
    pose0 = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    pose = torch.from_numpy(pose0.copy()).to(dev)
    stats = torch.zeros((iters, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    per = {r: [] for r in regions}
    wall = []
    for i in range(2 + a.icp_runs):
        pose.copy_(torch.from_numpy(pose0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.icp_dev(src, n, tgt, n, iters, np.inf, None, pose, None, stats)
        g.sync()
        w = (time.perf_counter() - t0) * 1e3
        got = {r: g.timing_read(r)[0] for r in regions}
        if i >= 2:
            wall.append(w)
            for r in regions:
                per[r].append(got[r])
    g.knn_check()
    st = stats.cpu().numpy()
    res["icp10"] = {"iters": iters, "runs": a.icp_runs, "wall_ms_med": med(wall),
                    "regions_ms_med": {r: med(per[r]) for r in regions},
                    "align_over_knn": round(float(np.median(per["align"]) /
                                                  (np.median(per["knn_build"]) +
                                                   np.median(per["knn_query"]))), 4),
                    "rms_first": float(st[0][1]), "rms_last": float(st[-1][1])}
    g.timing(False)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
