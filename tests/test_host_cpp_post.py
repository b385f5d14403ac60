"""svr_demo --post <operator>:<levels>: the C++ engine runs the HDR post pass (include/svr_post.h) behind every frame's
last pass and before the swapchain copy.  On the GPU the .color dump must be post_ref applied to the .color dump of the run
without the flag; the oracle has no post pass, so on the CPU the flag must fail loudly, as must a malformed one."""
import functools
import os

import numpy as np
import pytest

import post_ref as PR
import svr_testlib as T

W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_post_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--post", "aces:4")
    assert p.returncode != 0 and "--post: the library has no post pass (include/svr_post.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["aces", "aces:", "aces:9", "aces:-1", "aces:2x", "gamma:2", ":3"])
def test_a_malformed_post_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--post", arg)
    assert p.returncode != 0 and "--post: expected clamp|reinhard|aces:<levels 0..8>" in p.stdout


def test_post_excludes_views(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--post", "aces:4", "--views", "2")
    assert p.returncode != 0 and "--post: not with --views" in p.stdout


@pytest.mark.gpu
def test_deferred_post_dump_is_post_ref_of_the_plain_dump(tmp_path, hip):
    plain, posted = str(tmp_path / "plain"), str(tmp_path / "posted")
    knobs = ("--exposure", "2.5", "--bloom-threshold", "0.75", "--bloom-intensity", "0.5")
    p = run_demo(hip.path, plain, "--deferred", "1")
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, posted, "--deferred", "1", "--post", "aces:4", *knobs)
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(H, W, 4)
    got = np.fromfile(f"{posted}.color", dtype=np.uint16).reshape(H, W, 4)
    want = PR.run_ref(before, 2.5, 0.75, 0.5, 4, PR.ACES)["color"]
    assert not np.array_equal(want, before)
    assert np.array_equal(got, want)
    for k in ("depth", "opaque", "transparent", "scene"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{posted}.{k}", dtype=np.uint8)), k
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8), np.fromfile(f"{posted}.swapchain", dtype=np.uint8))
