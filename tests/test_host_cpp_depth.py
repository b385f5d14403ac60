"""svr_demo --depth-only 1: the C++ engine draws its frames as depth-only passes (include/svr_depth.h); the dumped depth
must be, bit for bit, what a normal run dumps, and the colour what the background alone leaves.  The oracle has no
depth-only pass, so on the CPU the flag must fail loudly."""
import functools

import numpy as np
import pytest

import svr_testlib as T

W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_depth_only_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--depth-only", "1")
    assert p.returncode != 0 and "no depth-only" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("retained", ["0", "1"])
def test_depth_only_dumps_the_depth_of_a_normal_run(tmp_path, hip, retained):
    full, dep = str(tmp_path / "full"), str(tmp_path / "depth")
    p = run_demo(hip.path, full, "--retained", retained)
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, dep, "--retained", retained, "--depth-only", "1")
    assert q.returncode == 0, q.stdout
    a = np.fromfile(f"{full}.depth", dtype=np.uint8)
    b = np.fromfile(f"{dep}.depth", dtype=np.uint8)
    assert a.size == b.size == W * H * 4 and np.array_equal(a, b), "depth"
    assert np.any(np.fromfile(f"{dep}.depth", dtype=np.float32) > 0)
    col = np.fromfile(f"{dep}.color", dtype=np.uint16).reshape(H, W, 4)
    assert np.all(col == col[0, 0]), "a depth-only frame leaves the background's colour"
