"""svr_demo --auto-exposure <key>:<adapt> (include/svr_exposure.h).  Without a GPU: the flag's refusals, through the oracle,
which has no auto-exposure.  On the GPU the swapchain the C++ engine writes is the one Python produces with the same calls
(tests/test_exposure_gpu.py)."""
import functools
import os

import pytest

import svr_testlib as T

W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_auto_exposure_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--post", "aces:4", "--auto-exposure", "0.18:1")
    assert p.returncode != 0 and "--auto-exposure: the library has no auto-exposure (include/svr_exposure.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


def test_auto_exposure_needs_post(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--auto-exposure", "0.18:1")
    assert p.returncode != 0 and "--auto-exposure: needs --post" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["0.18", "0.18:", ":1", "0:1", "-1:0.5", "0.18:1.5", "0.18:-0.1", "0.18:1x", "nan:1", "inf:1", "0.18:nan"])
def test_a_malformed_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--post", "aces:4", "--auto-exposure", arg)
    assert p.returncode != 0 and "--auto-exposure: expected <key > 0>:<adapt 0..1>" in p.stdout
