"""svr_demo --occlusion last|prepass: the C++ engine culls its frames against a depth pyramid (include/svr_occlusion.h),
of the previous frame's depth or of a depth-only pass of its occluders; with a static camera every dump must be, byte for
byte, what --occlusion off dumps.  The oracle has no pyramid, so on the CPU the flag must fail loudly."""
import functools

import numpy as np
import pytest

import svr_testlib as T

W, H = 160, 90
DUMPS = ("color", "depth", "swapchain", "opaque", "transparent", "scene")


run_demo = functools.partial(T.run_demo, width=W, height=H, frames=3)


@pytest.mark.parametrize("mode", ["last", "prepass"])
def test_occlusion_on_a_library_without_it_fails_loudly(tmp_path, oracle, mode):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--occlusion", mode)
    assert p.returncode != 0 and "no occlusion culling" in p.stdout


def test_an_unknown_mode_is_refused(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--occlusion", "sometimes")
    assert p.returncode != 0 and "off, last or prepass" in p.stdout


def test_off_on_the_oracle_runs(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--occlusion", "off", frames=1)
    assert p.returncode == 0, p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("retained", ["0", "1"])
@pytest.mark.parametrize("mode", ["last", "prepass"])
def test_culled_runs_dump_the_bytes_of_an_unculled_run(tmp_path, hip, mode, retained):
    off, cul = str(tmp_path / "off"), str(tmp_path / mode)
    p = run_demo(hip.path, off, "--retained", retained, "--occlusion", "off")
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, cul, "--retained", retained, "--occlusion", mode)
    assert q.returncode == 0, q.stdout
    for k in DUMPS:
        a = np.fromfile(f"{off}.{k}", dtype=np.uint8)
        b = np.fromfile(f"{cul}.{k}", dtype=np.uint8)
        assert a.size > 0 and np.array_equal(a, b), k
    assert np.any(np.fromfile(f"{cul}.depth", dtype=np.float32) > 0)
    r = run_demo(hip.path, str(tmp_path / "d"), "--occlusion", mode, "--depth-only", "1")
    assert r.returncode == 0, r.stdout
    assert np.array_equal(np.fromfile(f"{off}.depth", dtype=np.uint8), np.fromfile(str(tmp_path / "d") + ".depth", dtype=np.uint8))
