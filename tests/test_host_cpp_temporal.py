"""svr_demo --taa <blend> without a GPU: the oracle has no temporal pass, so the flag must fail loudly, as must a malformed
blend and the combinations the header rules out.  The GPU run is test_temporal_gpu.py::test_demo_taa_equals_the_python_path."""
import functools
import os

import pytest

import svr_testlib as T

W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_taa_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--taa", "0.1")
    assert p.returncode != 0 and "--taa: the library has no temporal pass (include/svr_temporal.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["0", "-0.1", "1.5", "nan", "inf", "0.1x", "x"])
def test_a_malformed_blend_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--taa", arg)
    assert p.returncode != 0 and "--taa: expected a blend in (0, 1]" in p.stdout


def test_taa_excludes_views_and_ranks(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--taa", "0.1", "--views", "2")
    assert p.returncode != 0 and "--taa: not with --views" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--taa", "0.1", "--ranks", "2")
    assert p.returncode != 0 and "--taa: not with --ranks" in p.stdout
