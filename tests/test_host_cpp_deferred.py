"""svr_demo --deferred 1: the C++ engine draws every frame as a G-buffer pass of the opaque objects, a lighting pass with
the scene's sun and ambient, and the transparent objects under SVR_DEPTH_LOAD (include/svr_attributes.h, svr_lighting.h,
svr_load.h); every dump must be, byte for byte, what the forward run dumps.  The oracle has none of the three, so on the
CPU the flag must fail loudly."""
import functools

import numpy as np
import pytest

import svr_testlib as T

W, H = 160, 90
DUMPS = ("color", "depth", "swapchain", "opaque", "transparent", "scene")


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_deferred_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1")
    assert p.returncode != 0 and "no attribute targets, lighting pass or depth loadOp" in p.stdout


@pytest.mark.parametrize("other", [("--retained", "1"), ("--depth-only", "1"), ("--views", "2"), ("--occlusion", "last")])
def test_deferred_excludes_the_other_modes(tmp_path, oracle, other):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", *other)
    assert p.returncode != 0 and "--deferred: not with" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("background", ["0", "1"])
def test_deferred_dumps_the_bytes_of_the_forward_run(tmp_path, hip, background):
    fwd, dfr = str(tmp_path / "forward"), str(tmp_path / "deferred")
    p = run_demo(hip.path, fwd, "--background", background)
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, dfr, "--background", background, "--deferred", "1")
    assert q.returncode == 0, q.stdout
    for k in DUMPS:
        a = np.fromfile(f"{fwd}.{k}", dtype=np.uint8)
        b = np.fromfile(f"{dfr}.{k}", dtype=np.uint8)
        assert a.size > 0 and np.array_equal(a, b), k
    assert np.fromfile(f"{dfr}.transparent", dtype=np.uint8).size > 0, "the scene has transparent objects"
    assert np.any(np.fromfile(f"{dfr}.depth", dtype=np.float32) > 0)
    draws = [line for line in (p.stdout + q.stdout).splitlines() if line.startswith("draws ")]
    assert len(draws) == 2 and draws[0].split()[:4] == draws[1].split()[:4], "the two passes count the forward run's draws and triangles"
