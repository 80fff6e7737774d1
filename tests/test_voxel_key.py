"""The cell and key rule of the voxel-grid downsampling (nav-slam_amd/csrc/
voxel_key.h) on the host: tests/voxel_key_driver.cpp is compiled against the
header with the address and undefined-behaviour sanitizers and run as a
stand-alone program (points in on stdin, cells and keys back). The checker is
numpy through tests/voxel_ref.py: np.floor((x - o) / v), the same three IEEE
operations."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from voxel_ref import NO_KEY, keys_of

CSRC = os.path.join(ROOT, "nav-slam_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "voxel_key_driver.cpp")
TOP = 2097151  # 2^21 - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxel_key") / "voxel_key_driver")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover", f"-I{CSRC}", DRIVER, "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(lines), capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return [list(map(int, ln.split())) for ln in r.stdout.splitlines()]
    return run


def hexes(*vals):
    return " ".join(float(v).hex() for v in vals)


def check_keys(driver, pts, voxel, origin, what):
    """the driver's cells and keys of pts against numpy's; returns (why, cells)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = driver([f"key {hexes(voxel, *origin, *p)}\n" for p in pts])
    keys, cells, why = keys_of(pts, voxel, origin)
    assert len(out) == len(pts), what
    for i, row in enumerate(out):
        assert row[0] == why[i], (what, i, pts[i], row)
        assert row[1:4] == cells[i].tolist(), (what, i, pts[i], row)
        assert row[4] == int(keys[i]), (what, i, pts[i], row)
        assert row[5:8] == cells[i].tolist(), (what, i, "unpack", row)   # -1s when dropped
    return why, cells


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (-3.5, 0.0, 12.25)])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_faces(driver, origin, axis):
    # o + i * 0.1 is rarely the face itself: the cell is whatever the three
    # rounded operations give, and numpy's are the same three
    o = np.array(origin)
    pts = np.tile(o + 0.05, (100, 1))
    pts[:, axis] = o[axis] + np.arange(100) * 0.1
    why, cells = check_keys(driver, pts, 0.1, origin, f"faces axis {axis}")
    assert (why == 0).all()
    assert (np.abs(cells[:, axis] - np.arange(100)) <= 1).all()


def test_key_range(driver):
    o = (0.0, 0.0, 0.0)
    pts = []
    for a in range(3):
        for x in (float(TOP), TOP + 0.5, TOP + 1.0, -1.0, -0.5, np.nextafter(0.0, -1.0)):
            p = [0.5, 0.5, 0.5]
            p[a] = x
            pts.append(p)
    pts.append([TOP + 0.5] * 3)
    why, cells = check_keys(driver, pts, 1.0, o, "key range")
    assert why.tolist() == [0, 0, 2, 2, 2, 2] * 3 + [0]
    assert cells[-1].tolist() == [TOP] * 3
    keys = keys_of(pts, 1.0, o)[0]
    assert int(keys[-1]) == 2 ** 63 - 1 and keys[2] == NO_KEY


def test_non_finite_and_zeros(driver):
    pts = []
    for a in range(3):
        for x in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            p = [1.5, 2.5, 3.5]
            p[a] = x
            pts.append(p)
    why, cells = check_keys(driver, pts, 1.0, (0.0, 0.0, 0.0), "non-finite")
    assert why.tolist() == [1, 1, 1, 0, 0] * 3
    assert cells[3].tolist() == [0, 2, 3] and cells[4].tolist() == [0, 2, 3]   # +0 and -0
    # finite coordinates whose offset overflows or whose quotient is huge: out of range
    big = [[1e308, 0.0, 0.0], [0.0, -1e308, 0.0], [0.0, 0.0, 1e300]]
    why, _ = check_keys(driver, big, 1e-300, (-1e308, 1e308, 0.0), "overflow")
    assert why.tolist() == [2, 2, 2]


def test_argument_rule(driver):
    rows = [(1.0, (0.0, 0.0, 0.0)), (0.0, (0.0, 0.0, 0.0)), (-1.0, (0.0, 0.0, 0.0)),
            (np.nan, (0.0, 0.0, 0.0)), (np.inf, (0.0, 0.0, 0.0)), (5e-324, (0.0, 0.0, 0.0)),
            (1.0, (np.nan, 0.0, 0.0)), (1.0, (0.0, np.inf, 0.0)), (1.0, (0.0, 0.0, -np.inf))]
    out = driver([f"args {hexes(v, *o)}\n" for v, o in rows])
    assert out == [[1, 1], [0, 1], [0, 1], [0, 1], [0, 1], [1, 1], [1, 0], [1, 0], [1, 0]]
