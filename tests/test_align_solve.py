"""The closed-form rigid solver of the align step (nav-slam_amd/csrc/
align_solve.h) on the host: tests/align_solve_driver.cpp is compiled against
the header with the address and undefined-behaviour sanitizers and run as a
stand-alone program (moments in on stdin, poses back). The checker is the
numpy restatement ref_align (tests/reg_ref.py, Kabsch by SVD); the reference
project has no rotation fit to compare with."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from reg_ref import EPS, ref_align, rot

CSRC = os.path.join(ROOT, "nav-slam_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "align_solve_driver.cpp")


def tolerances(s, d, coord_max):
    kappa = s[0] / (s[1] + d * s[2])
    tol_R = 1024 * EPS * kappa
    return kappa, tol_R, (2 * tol_R + 64 * EPS) * coord_max


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_solve") / "align_solve_driver")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover", f"-I{CSRC}", DRIVER, "-o", exe], check=True)

    def run(cmd, *arrays):
        vals = np.concatenate([np.asarray(a, np.float64).ravel() for a in arrays])
        line = cmd + " " + " ".join(float(v).hex() for v in vals) + "\n"
        r = subprocess.run([exe], input=line, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return np.array([float.fromhex(w) for w in r.stdout.split()])
    return run


def solve(driver, m):
    out = driver("solve", m)
    assert out.shape == (16,)
    return out[:9].reshape(3, 3), out[9:12], out[12:]


T0 = np.array([120.0, -40.0, 5.0])


def _cube(rng, n=200):
    return rng.uniform(-500.0, 500.0, (n, 3))


def _slab(seed):
    # 50 points, 1 mm thick, with 3 mm of noise on the target side: the noise
    # dominates the thin axis, so the sign of det(H) depends on the seed
    rng = np.random.default_rng(seed)
    p = rng.uniform(-500.0, 500.0, (50, 3)) * np.array([1.0, 1.0, 0.001])
    q = p @ rot((1, 2, 3), 25.0).T + T0 + rng.normal(0.0, 3.0, (50, 3))
    return p, q


def _cases():
    rng = np.random.default_rng(7)
    c = {}
    p = _cube(rng)
    c["cube"] = (p, p @ rot((1, 2, 3), 25.0).T + T0)
    c["identity"] = (p, p.copy())
    c["half_turn_z"] = (p, p @ rot((0, 0, 1), 180.0).T + T0)
    c["half_turn_111"] = (p, p @ rot((1, 1, 1), 180.0).T + T0)
    c["almost_half_turn"] = (p, p @ rot((3, -1, 2), 179.999).T + T0)
    flat = _cube(rng) * np.array([1.0, 1.0, 0.0])
    c["planar"] = (flat, flat @ rot((1, 2, 3), 25.0).T + T0)
    c["slab_neg_det_a"] = _slab(SLAB_SEEDS[0])
    c["slab_neg_det_b"] = _slab(SLAB_SEEDS[1])
    line = _cube(rng) * np.array([1.0, 1.0 / 1100.0, 1.0 / 1100.0])  # kappa ~ 6e5
    c["near_collinear"] = (line, line @ rot((1, 2, 3), 25.0).T + T0)
    return c


# seeds of _slab whose H has a negative determinant (asserted by the test)
SLAB_SEEDS = (1, 8)
CASES = ["cube", "identity", "half_turn_z", "half_turn_111", "almost_half_turn", "planar",
         "slab_neg_det_a", "slab_neg_det_b", "near_collinear"]


@pytest.mark.parametrize("name", CASES)
def test_solver_matches_restatement(driver, name):
    p, q = _cases()[name]
    Rr, tr, s, d, m = ref_align(p, q)
    kappa, tol_R, tol_t = tolerances(s, d, max(np.abs(p).max(), np.abs(q).max()))
    assert kappa <= 1e6, kappa
    if name.startswith("slab"):
        assert np.linalg.det(m[8:17].reshape(3, 3)) < 0 and d < 0
    if name == "near_collinear":
        assert kappa > 1e5
    R, t, st = solve(driver, m)
    errR = np.abs(R - Rr).max()
    print(f"{name}: kappa {kappa:.3g} |R-Rref| {errR:.3g} (tol {tol_R:.3g}) "
          f"|t-tref| {np.abs(t - tr).max():.3g} (tol {tol_t:.3g})")
    assert errR <= tol_R
    assert np.abs(t - tr).max() <= tol_t
    assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * EPS
    assert np.linalg.det(R) > 0
    n = len(p)
    assert st[0] == n and st[3] == 0
    assert st[1] == np.sqrt(m[7] / n)
    after = np.sqrt((((p @ Rr.T + tr) - q) ** 2).sum() / n)
    assert abs(st[2] - after) <= np.sqrt(1024 * EPS * (m[17] + m[18]) / n)


def test_zero_H_gives_identity(driver):
    m = np.zeros(20)
    m[0] = 10
    m[1:4] = (1.0, 2.0, 3.0)
    m[4:7] = (11.0, 22.0, 33.0)
    m[7] = 10 * (10.0 ** 2 + 20.0 ** 2 + 30.0 ** 2)
    R, t, st = solve(driver, m)
    assert np.array_equal(R, np.eye(3))
    assert np.array_equal(t, [10.0, 20.0, 30.0])
    assert st[0] == 10 and st[2] == 0.0


@pytest.mark.parametrize("n", [0, 1, 2])
def test_too_few_pairs_give_identity(driver, n):
    rng = np.random.default_rng(n)
    p = _cube(rng, n)
    q = p @ rot((1, 2, 3), 25.0).T + T0
    m = ref_align(p, q)[4]
    m[19] = 4.0
    R, t, st = solve(driver, m)
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    rms = np.sqrt(m[7] / n) if n else 0.0
    assert np.array_equal(st, [n, rms, rms, 4.0])


def test_pose_compose_bit_equal(driver):
    rng = np.random.default_rng(11)
    for _ in range(4):
        d = np.concatenate([rot(rng.normal(size=3), rng.uniform(0, 180)).ravel(),
                            rng.uniform(-1e3, 1e3, 3)])
        P = np.concatenate([rot(rng.normal(size=3), rng.uniform(0, 180)).ravel(),
                            rng.uniform(-1e7, 1e7, 3)])
        want = np.empty(12)
        for i in range(3):
            a, b, c = d[3 * i], d[3 * i + 1], d[3 * i + 2]
            for j in range(3):
                want[3 * i + j] = (a * P[j] + b * P[3 + j]) + c * P[6 + j]
            want[9 + i] = ((a * P[9] + b * P[10]) + c * P[11]) + d[9 + i]
        got = driver("compose", d, P)
        assert np.array_equal(got, want)
