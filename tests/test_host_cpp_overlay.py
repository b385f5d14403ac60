"""svr_demo --stats-overlay 1 (include/svr_overlay.h): behind the last frame the C++ engine copies the colour target to a
swapchain image and draws the reference's stats window onto it with svr_draw_overlay.  On the GPU the .swapchain dump must be
overlay_ref applied to the .swapchain dump of the run without the flag, with the list rebuilt in Python from .overlay.txt;
the oracle has no overlay pass, so on the CPU the flag must fail loudly."""
import functools
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import overlay_ref as R
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_stats_overlay_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--stats-overlay", "1")
    assert p.returncode != 0 and "--stats-overlay: the library has no overlay pass (include/svr_overlay.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.swapchain"))


@pytest.mark.parametrize("other", [("--views", "2"), ("--ranks", "2")])
def test_stats_overlay_excludes_views_and_ranks(tmp_path, oracle, other):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--stats-overlay", "1", *other)
    assert p.returncode != 0 and "--stats-overlay: not with --views or --ranks" in p.stdout


def rebuilt_list(text, hip):
    """the builder calls of .overlay.txt, made again in Python"""
    font = A.overlay_font(hip)
    b = pkg.overlay.ListBuilder(font)
    lines = text.splitlines()
    for line in lines:
        kind, rest = line.split(" ", 1)
        if kind == "window":
            x, y, w, h, title = rest.split(" ", 4)
            b.window(int(x), int(y), int(w), int(h), title)
        else:
            assert kind == "text"
            x, y, string = rest.split(" ", 2)
            b.text(int(x), int(y), string, (255, 255, 255, 255))
    vertices, indices, cmds = b.arrays()
    return lines, R.make_list(vertices, indices, cmds, textures=[(font[0], 96, 48, A.OVERLAY_TEX_A8)])


@pytest.mark.gpu
def test_stats_overlay_dump_is_overlay_ref_of_the_plain_dump(tmp_path, hip):
    plain, drawn = str(tmp_path / "plain"), str(tmp_path / "drawn")
    p = run_demo(hip.path, plain)
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, drawn, "--stats-overlay", "1")
    assert q.returncode == 0, q.stdout
    lines, lst = rebuilt_list(open(f"{drawn}.overlay.txt").read(), hip)
    assert lines[0] == "window 10 10 150 64 stats" and len(lines) == 6
    for line, pattern in zip(lines[1:], [r"frametime -?\d+\.\d{6} ms", r"draw time -?\d+\.\d{6} ms", r"update time -?\d+\.\d{6} ms", r"triangles \d+", r"draws \d+"]):
        assert re.fullmatch(r"text \d+ \d+ " + pattern, line), line
    counts = re.search(r"draws (\d+) triangles (\d+)", q.stdout)
    assert lines[4].endswith(f"triangles {counts.group(2)}") and lines[5].endswith(f"draws {counts.group(1)}")
    before = np.fromfile(f"{plain}.swapchain", dtype=np.uint32).reshape(H, W)
    got = np.fromfile(f"{drawn}.swapchain", dtype=np.uint32).reshape(H, W)
    want, count, _ = R.run_ref(before, R.BGRA, lst)
    assert (count > 0).sum() >= 150 * 64 and count.max() >= 3
    assert np.array_equal(got, want)
    assert np.array_equal(got[count == 0], before[count == 0])
    for k in ("color", "depth"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{drawn}.{k}", dtype=np.uint8)), k
