"""Timing of the registration: surface normals, the point-to-point and
point-to-plane steps and their ICP loops. GPU only.

Workloads: uniform_pair() at 1,048,576 points a side and l9_pair() at
128 x 2048. Medians over the timed calls after warm-up, HIP events from the
timing hook. Per workload it reports
  * the "normals" region (k_normals on the target's own 8-NN rows), its bytes
    model (per point: 32 B idx + 192 B gathers + 24 B self + 32 B out) and
    that rate as a fraction of the navgpu_stream_copy_dev ceiling of the run;
  * the "align_plane" region on k = 1 rows (per query, pass B: 24 B src + 4 B
    idx + 8 B dist + 24 B target + 24 B normal + 8 B curvature = 92 B; pass A
    reads the src, idx, dist and curvature: 44 B);
  * the point-to-point "align" region (pass A, finish, pass B, solve; per
    query and pass: 24 B src + 4 B idx + 8 B dist + a 24-B gather) on k = 1
    rows and on k = 8 rows, of which the step reads slot 0;
  * a 10-iteration icp_plane_dev against a 10-iteration icp_dev, split into
    regions (k-NN build and query, transform, step), and their wall times.
The keys of the former align_bench.py output (profiles/align/) are those of
the uniform_1M workload; those of plane_bench.py (profiles/plane/) are kept.
Writes the JSON to --out (default profiles/registration/bench.json) and prints
it on one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nav-slam_amd"))
from navslam.gpu import NavGpu  # noqa: E402
from navslam.synth import l9_pair, uniform_pair  # noqa: E402

KN = 8
NORMALS_BYTES_PER_POINT = 4 * KN + 24 * KN + 24 + 32
PLANE_BYTES_PASS_A = 24 + 4 + 8 + 8
PLANE_BYTES_PASS_B = 24 + 4 + 8 + 24 + 24 + 8
PLANE_BYTES_PER_QUERY = PLANE_BYTES_PASS_A + PLANE_BYTES_PASS_B
ALIGN_BYTES_PER_QUERY_PASS = 24 + 4 + 8 + 24
ALIGN_PASSES = 2


def med(v):
    return round(float(np.median(v)), 5)


def region_stats(ts, model, copy_gbs):
    gbs = model / (np.median(ts) * 1e-3) / 1e9
    return {"ms_med": med(ts), "ms_min": round(float(np.min(ts)), 5),
            "ms_p90": round(float(np.percentile(ts, 90)), 5), "bytes_model": model,
            "GBps_model": round(gbs, 1), "fraction_of_stream_copy": round(gbs / copy_gbs, 4)}


def timed(g, region, calls, warmup, fn):
    g.timing_select(region)
    ts = []
    for i in range(warmup + calls):
        fn()
        g.sync()
        ms, cnt = g.timing_read(region)
        assert cnt == 1
        if i >= warmup:
            ts.append(ms)
    return ts


def workload(g, torch, dev, s, t, a, copy_gbs):
    n = len(s)
    src = torch.from_numpy(np.ascontiguousarray(s)).to(dev)
    tgt = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    nrm = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    curv = torch.zeros(n, dtype=torch.float64, device=dev)
    out18 = torch.zeros(18, dtype=torch.float64, device=dev)
    idx8 = torch.zeros((n, KN), dtype=torch.int32, device=dev)
    dist8 = torch.zeros((n, KN), dtype=torch.float64, device=dev)
    idx1 = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    dist1 = torch.zeros((n, 1), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    res = {"points": n}
    vp = (0.0, 0.0, 0.0)

    g.timing_select("normals")
    g.knn_dev(tgt, n, tgt, n, KN, idx8, dist8)
    g.sync()
    ts = timed(g, "normals", a.calls, a.warmup,
               lambda: g.normals_dev(tgt, n, idx8, KN, KN, vp, nrm, curv))
    res["normals_k8"] = region_stats(ts, NORMALS_BYTES_PER_POINT * n, copy_gbs)
    res["normals_k8"]["invalid"] = int(torch.isnan(curv).sum().item())

    g.knn_dev(tgt, n, src, n, 1, idx1, dist1)
    g.sync()
    ts = timed(g, "align_plane", a.calls, a.warmup,
               lambda: g.align_plane_dev(src, n, tgt, n, nrm, curv, idx1, dist1, 1, np.inf,
                                         np.inf, None, out18, None, out18[12:]))
    o = out18.cpu().numpy()
    res["align_plane_k1"] = region_stats(ts, PLANE_BYTES_PER_QUERY * n, copy_gbs)
    res["align_plane_k1"].update(pairs=int(o[12]), rms_before=float(o[13]),
                                 rms_after=float(o[14]), solved=int(o[16]),
                                 min_pivot=float(o[17]))
    g.knn_dev(tgt, n, src, n, KN, idx8, dist8)  # the rows of the k = 8-stride align
    g.sync()
    for k, idx, dist in ((1, idx1, dist1), (KN, idx8, dist8)):
        ts2 = timed(g, "align", a.calls, a.warmup,
                    lambda: g.align_dev(src, n, tgt, n, idx, dist, k, np.inf, None, out18, None,
                                        out18[12:]))
        o = out18.cpu().numpy()
        res[f"align_k{k}"] = region_stats(ts2, ALIGN_PASSES * ALIGN_BYTES_PER_QUERY_PASS * n,
                                          copy_gbs)
        res[f"align_k{k}"].update(pairs=int(o[12]), rms_before=float(o[13]),
                                  rms_after=float(o[14]))
    res["plane_over_align"] = round(res["align_plane_k1"]["ms_med"] /
                                    res["align_k1"]["ms_med"], 4)

    # 10 iterations of each ICP, every region timed
    g.timing_select(None)
    iters = 10
    pose0 = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    pose = torch.from_numpy(pose0.copy()).to(dev)
    stats = torch.zeros((iters, 6), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for kind, step in (("icp_plane10", "align_plane"), ("icp10", "align")):
        regions = ("icp_transform", "knn_build", "knn_query", step)
        per = {r: [] for r in regions}
        wall = []
        for i in range(2 + a.icp_runs):
            pose.copy_(torch.from_numpy(pose0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if step == "align":
                g.icp_dev(src, n, tgt, n, iters, np.inf, None, pose, None, stats)
            else:
                g.icp_plane_dev(src, n, tgt, n, nrm, curv, iters, np.inf, np.inf, None, pose,
                                None, stats)
            g.sync()
            w = (time.perf_counter() - t0) * 1e3
            got = {r: g.timing_read(r)[0] for r in regions}
            if i >= 2:
                wall.append(w)
                for r in regions:
                    per[r].append(got[r])
        g.knn_check()
        st = stats.cpu().numpy().ravel()
        width = 4 if step == "align" else 6
        res[kind] = {"iters": iters, "runs": a.icp_runs, "wall_ms_med": med(wall),
                     "regions_ms_med": {r: med(per[r]) for r in regions},
                     "rms_first": float(st[1]), "rms_last": float(st[width * (iters - 1) + 1])}
        if step == "align":
            res[kind]["align_over_knn"] = round(
                float(np.median(per["align"]) / (np.median(per["knn_build"]) +
                                                 np.median(per["knn_query"]))), 4)
    res["icp_plane_over_icp_wall"] = round(res["icp_plane10"]["wall_ms_med"] /
                                           res["icp10"]["wall_ms_med"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "registration", "bench.json"))
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--icp-runs", type=int, default=10)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    g = NavGpu(0)
    res = {"calls": a.calls, "warmup": a.warmup, "kn": KN,
           "bytes_model_normals_per_point": NORMALS_BYTES_PER_POINT,
           "bytes_model_plane_per_query": PLANE_BYTES_PER_QUERY,
           "bytes_model_plane_pass_b": PLANE_BYTES_PASS_B,
           "bytes_model_align_per_query_pass": ALIGN_BYTES_PER_QUERY_PASS,
           "bytes_model_per_query_pass": ALIGN_BYTES_PER_QUERY_PASS, "passes": ALIGN_PASSES}

    # the measured HBM ceiling: a streaming device-to-device copy
    nb = 256 << 20
    ca = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    cb = torch.ones(nb // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    g.timing(True)
    ts = timed(g, "stream_copy", 20, a.warmup, lambda: g.stream_copy_dev(ca, cb, nb))
    copy_gbs = 2 * nb / (np.median(ts) * 1e-3) / 1e9
    res["stream_copy"] = {"bytes_each_way": nb, "ms_med": med(ts), "GBps": round(copy_gbs, 1)}
    del ca, cb

    s, t = uniform_pair(512, 2048)
    res["uniform_1M"] = workload(g, torch, dev, s.reshape(-1, 3), t.reshape(-1, 3), a, copy_gbs)
    s, t = l9_pair(128, 2048)
    res["l9_128x2048"] = workload(g, torch, dev, s.reshape(-1, 3), t.reshape(-1, 3), a, copy_gbs)
    g.timing(False)
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
