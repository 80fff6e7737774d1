"""A mask and a non-identity initial pose through the ICP host entry points
(gpu.icp, gpu.icp_plane): each must equal, byte for byte, the same inputs
uploaded as torch tensors and run through the device-pointer entry points.
Both paths run the same kernels on the same nq, and the sums are reproducible
by construction (DESIGN.md §10 "Determinism"), so the equality is exact."""
import numpy as np
import pytest

from reg_ref import l9_clouds, rot

pytestmark = pytest.mark.gpu

ITERS = 3
GATE = 150.0
INIT = (rot((1, 2, 3), 5.0), np.array([10.0, -5.0, 2.0]))


@pytest.fixture(scope="module")
def gpu():
    from navslam.gpu import NavGpu
    g = NavGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def case():
    src, tgt = l9_clouds()
    mask = (np.random.default_rng(41).random(len(src)) < 0.8).astype(np.int32)
    assert 0.75 * len(src) < mask.sum() < 0.85 * len(src)   # drops about a fifth
    return src, tgt, mask


def device_inputs(src, tgt, mask, width):
    import torch
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pose = to(np.concatenate([INIT[0].ravel(), INIT[1]]))
    hist = torch.zeros((ITERS, 12), dtype=torch.float64, device=dev)
    stats = torch.zeros((ITERS, width), dtype=torch.float64, device=dev)
    return to(src), to(tgt), to(mask), pose, hist, stats


def check_equal(host, pose, hist, stats, mask, n_src):
    R, t, h_stats, h_hist = host
    assert np.concatenate([R.ravel(), t]).tobytes() == pose.cpu().numpy().tobytes()
    assert h_hist.tobytes() == hist.cpu().numpy().tobytes()
    assert h_stats.tobytes() == stats.cpu().numpy().tobytes()
    print("pairs per iteration:", h_stats[:, 0], "mask", mask.sum(), "of", n_src)
    assert 0 < h_stats[0][0] <= mask.sum()
    assert h_stats[0][0] < n_src


def test_icp_host_equals_dev_with_mask_and_init(gpu, case):
    import torch
    src, tgt, mask = case
    host = gpu.icp(src, tgt, iters=ITERS, max_dist=GATE, mask=mask, init=INIT)
    d_src, d_tgt, d_mask, pose, hist, stats = device_inputs(src, tgt, mask, 4)
    torch.cuda.synchronize()
    gpu.icp_dev(d_src, len(src), d_tgt, len(tgt), ITERS, GATE, d_mask, pose, hist, stats)
    gpu.sync()
    gpu.knn_check()
    check_equal(host, pose, hist, stats, mask, len(src))


def test_icp_plane_host_equals_dev_with_mask_and_init(gpu, case):
    import torch
    src, tgt, mask = case
    host = gpu.icp_plane(src, tgt, tgt_normals=None, iters=ITERS, max_dist=GATE, mask=mask,
                         init=INIT, kn=8)
    d_src, d_tgt, d_mask, pose, hist, stats = device_inputs(src, tgt, mask, 6)
    d_n = torch.zeros((len(tgt), 3), dtype=torch.float64, device=d_tgt.device)
    d_c = torch.zeros(len(tgt), dtype=torch.float64, device=d_tgt.device)
    torch.cuda.synchronize()
    gpu.cloud_normals_dev(d_tgt, len(tgt), 8, None, d_n, d_c)
    gpu.icp_plane_dev(d_src, len(src), d_tgt, len(tgt), d_n, d_c, ITERS, GATE, np.inf, d_mask,
                      pose, hist, stats)
    gpu.sync()
    gpu.knn_check()
    check_equal(host, pose, hist, stats, mask, len(src))
