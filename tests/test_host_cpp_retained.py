"""svr_demo --retained 1: the C++ engine keeps its draw context in a draw list (include/svr_draw_list.h) and draws it
with svr_draw_list; the frames must be those of the svr_draw_geometry path, bit for bit.  The oracle has no draw
lists, so on the CPU the flag must fail loudly."""
import numpy as np
import pytest

import svr_testlib as T

W, H = 160, 90


def run_demo(lib_path, prefix, retained, frames=3):
    return T.run_demo(lib_path, prefix, "--retained", "1" if retained else "0", width=W, height=H, frames=frames)


def test_retained_on_a_library_without_draw_lists_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), True)
    assert p.returncode != 0 and "no draw lists" in p.stdout


@pytest.mark.gpu
def test_retained_gives_the_same_image(tmp_path, hip):
    out = {}
    for retained in (False, True):
        prefix = str(tmp_path / f"demo{int(retained)}")
        p = run_demo(hip.path, prefix, retained)
        assert p.returncode == 0, p.stdout
        out[retained] = {k: np.fromfile(prefix + "." + k, dtype=np.uint8) for k in ("color", "depth", "swapchain")}
    for k in ("color", "depth", "swapchain"):
        assert out[True][k].size > 0 and np.array_equal(out[True][k], out[False][k]), k
