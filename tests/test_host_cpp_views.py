"""svr_demo --views N: the C++ engine draws N cameras (yaw stepped by 360/N) in one multiview pass
(include/svr_views.h); every dumped layer must be, bit for bit, what a single-camera run with that view's yaw leaves
in its colour and depth targets.  The oracle has no multiview, so on the CPU the flag must fail loudly."""
import functools
import re

import numpy as np
import pytest

import svr_testlib as T

W, H = 160, 90  # 90 rows: every layer's last tile row is partial


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_views_on_a_library_without_multiview_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--views", "2")
    assert p.returncode != 0 and "no multiview" in p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("n,retained", [(1, "0"), (2, "0"), (6, "1"), (16, "0")])
def test_views_match_single_camera_runs(tmp_path, hip, n, retained):
    prefix = str(tmp_path / "views")
    p = run_demo(hip.path, prefix, "--views", str(n), "--retained", retained)
    assert p.returncode == 0, p.stdout
    yaws = dict((int(k), v) for k, v in re.findall(r"^view (\d+) yaw (\S+)$", p.stdout, flags=re.M))
    assert sorted(yaws) == list(range(n))
    for k in range(n):
        one = str(tmp_path / f"single{k}")
        q = run_demo(hip.path, one, "--yaw", yaws[k], "--retained", retained)
        assert q.returncode == 0, q.stdout
        for part in ("color", "depth"):
            a = np.fromfile(f"{prefix}.view{k}.{part}", dtype=np.uint8)
            b = np.fromfile(f"{one}.{part}", dtype=np.uint8)
            assert a.size == b.size > 0 and np.array_equal(a, b), f"view {k} of {n}: {part}"
