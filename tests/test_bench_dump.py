"""bench.py as a program on the GPU: a plain run times --steps steps and
leaves the extras to --full, and --dump-outputs writes what its last timed
step computed, checked here against the oracle on that step's pair."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dump_of_the_last_step(tmp_path, orc):
    from navslam.synth import uniform_pair
    R, Cc, k, steps, warmup, npairs = 32, 256, 8, 3, 1, 2
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(steps), "--warmup", str(warmup), "--rows", str(R),
                        "--cols", str(Cc), "--resident-pairs", str(npairs),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    out = lines[0]
    assert out["steps"] == steps and out["warmup"] == warmup and out["full"] is False
    assert out["ms_per_step"] > 0 and out["unit"] == "matches/s" and out["dtype"] == "f64"
    # value = matches per step over the time of a step (the line rounds
    # ms_per_step to 1e-4 ms)
    assert out["value"] == pytest.approx(R * Cc / (out["ms_per_step"] * 1e-3),
                                         rel=0.5e-4 / out["ms_per_step"] + 1e-6)
    # the runs of their own are --full's
    assert out["cpu_baseline"] is None and out["kernel_us_isolated"] is None
    assert "stream_copy" not in (out["roofline"] or {})
    # the last timed step is step warmup + steps - 1 of the rotation over the
    # resident pairs; pair j has seeds (1 + 1000 j, 2 + 1000 j)
    j = (warmup + steps - 1) % npairs
    src, tgt = uniform_pair(R, Cc, seed_src=1 + 1000 * j, seed_tgt=2 + 1000 * j)
    got = {n: np.load(d / (n + ".npy")) for n in ("src_mask", "tgt_mask", "nn_idx", "nn_dist")}
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in got)
    assert got["nn_dist"].dtype == np.float64
    assert all(got[n].dtype == np.float32 for n in ("src_mask", "tgt_mask", "nn_idx"))
    ri, rd = orc.knn_brute(tgt, src, k)
    np.testing.assert_array_equal(got["nn_idx"], ri)
    np.testing.assert_array_equal(got["nn_dist"], rd)
    np.testing.assert_array_equal(got["src_mask"], orc.extract_feature(src))
    np.testing.assert_array_equal(got["tgt_mask"], orc.extract_feature(tgt))
