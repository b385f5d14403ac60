"""svr_demo --render-scale <s> [--upscale <sharpness>|off] (include/svr_upscale.h): the C++ engine creates its context at the
reference's render extent and presents into a window-sized swapchain image, through svr_upscale_to_swapchain's arithmetic or,
with off, the scaled svr_copy_to_swapchain.  On the GPU the .swapchain dump must be what the Python binding gives for the
dumped colour target; the oracle has no upscaled present, so on the CPU --upscale must fail loudly and off must work."""
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as g
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
W, H = 128, 72
BGRA = 0


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_upscale_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--render-scale", "0.5", "--upscale", "0.5")
    assert p.returncode != 0 and "--upscale: the library has no upscaled present (include/svr_upscale.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.swapchain"))


@pytest.mark.parametrize("args,code,needle", [(("--render-scale", "0"), 2, "--render-scale: expected a scale in (0, 1]"),
                                              (("--render-scale", "1.5"), 2, "--render-scale: expected a scale in (0, 1]"),
                                              (("--render-scale", "half"), 2, "--render-scale: expected a scale in (0, 1]"),
                                              (("--upscale", "2"), 2, "--upscale: expected a sharpness in [0, 1] or off"),
                                              (("--render-scale", "0.5", "--views", "2"), 1, "--render-scale: not with --views or --ranks"),
                                              (("--upscale", "0.5", "--ranks", "2"), 1, "--upscale: not with --views or --ranks")])
def test_bad_arguments_are_refused(tmp_path, oracle, args, code, needle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), *args)
    assert p.returncode == code and needle in p.stdout, p.stdout


def test_render_scale_without_upscale_is_the_scaled_blit_of_the_smaller_frame(tmp_path, oracle):
    """the reference's behaviour, on the oracle: the targets have the render extent, the swapchain image the window's"""
    prefix = str(tmp_path / "demo")
    p = run_demo(oracle.path, prefix, "--render-scale", "0.5", "--upscale", "off")
    assert p.returncode == 0 and "render extent 64x36" in p.stdout, p.stdout
    assert os.path.getsize(prefix + ".color") == 64 * 36 * 8 and os.path.getsize(prefix + ".depth") == 64 * 36 * 4
    swap = np.fromfile(prefix + ".swapchain", np.uint8)
    assert swap.size == W * H * 4 and len(np.unique(swap.view(np.uint32))) > 20
    q = run_demo(oracle.path, str(tmp_path / "odd"), "--render-scale", "0.667")
    rw, rh = pkg.glmath.render_extent(W, H, 0.667)
    assert q.returncode == 0 and f"render extent {rw}x{rh}" in q.stdout and (rw, rh) == (85, 48), q.stdout


def python_context(hip, prefix, rw, rh):
    """a context of the binding's over the demo's dumped colour target"""
    import torch
    color = torch.from_numpy(np.fromfile(prefix + ".color", np.int16).reshape(rh, rw, 4).copy()).cuda()
    depth = torch.zeros((rh, rw), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = hip.create(rw, rh)
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    return r, (color, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", ["0.5", "0.667"])
def test_demo_dumps_the_bytes_the_python_path_gives(tmp_path, hip, scale):
    pytest.importorskip("torch")
    rw, rh = pkg.glmath.render_extent(W, H, float(scale))
    up, off = str(tmp_path / "up"), str(tmp_path / "off")
    p = run_demo(hip.path, up, "--render-scale", scale, "--upscale", "0.5")
    assert p.returncode == 0 and f"render extent {rw}x{rh}" in p.stdout, p.stdout
    q = run_demo(hip.path, off, "--render-scale", scale, "--upscale", "off")
    assert q.returncode == 0, q.stdout
    assert np.array_equal(np.fromfile(up + ".color", np.uint8), np.fromfile(off + ".color", np.uint8))
    r, keep = python_context(hip, up, rw, rh)
    want_up = r.read_upscaled(W, H, BGRA, 0.5, 0)
    want_off = r.read_swapchain(W, H, BGRA)
    r.close()
    got_up = np.fromfile(up + ".swapchain", np.uint8).reshape(H, W, 4)
    got_off = np.fromfile(off + ".swapchain", np.uint8).reshape(H, W, 4)
    assert np.array_equal(got_up, want_up)
    assert np.array_equal(got_off, want_off)
    assert (got_up != got_off).any() and len(np.unique(got_up.view(np.uint32))) > 50


def rebuilt_list(text, hip):
    """the builder calls of .overlay.txt, made again in Python (as tests/test_host_cpp_overlay.py does)"""
    import overlay_ref
    font = A.overlay_font(hip)
    b = pkg.overlay.ListBuilder(font)
    for line in text.splitlines():
        kind, rest = line.split(" ", 1)
        if kind == "window":
            x, y, w, h, title = rest.split(" ", 4)
            b.window(int(x), int(y), int(w), int(h), title)
        else:
            assert kind == "text"
            x, y, string = rest.split(" ", 2)
            b.text(int(x), int(y), string, (255, 255, 255, 255))
    vertices, indices, cmds = b.arrays()
    return overlay_ref.make_list(vertices, indices, cmds, textures=[(font[0], 96, 48, A.OVERLAY_TEX_A8)])


@pytest.mark.gpu
def test_stats_overlay_draws_over_the_upscaled_image_at_window_resolution(tmp_path, hip):
    """the .swapchain dump is overlay_ref applied to the window-sized upscaled image of the run without the flag"""
    pytest.importorskip("torch")
    import overlay_ref
    plain, drawn = str(tmp_path / "plain"), str(tmp_path / "drawn")
    p = run_demo(hip.path, plain, "--render-scale", "0.5", "--upscale", "0.5")
    q = run_demo(hip.path, drawn, "--render-scale", "0.5", "--upscale", "0.5", "--stats-overlay", "1")
    assert p.returncode == 0 and q.returncode == 0, p.stdout + q.stdout
    before = np.fromfile(plain + ".swapchain", np.uint32).reshape(H, W)
    got = np.fromfile(drawn + ".swapchain", np.uint32).reshape(H, W)
    want, count, _ = overlay_ref.run_ref(before, overlay_ref.BGRA, rebuilt_list(open(drawn + ".overlay.txt").read(), hip))
    assert (count > 0).sum() >= (W - 10) * (H - 10) and count.max() >= 3  # the window at (10, 10), 150 x 64, cut by the 128 x 72 image
    assert np.array_equal(got, want)
    assert np.array_equal(got[count == 0], before[count == 0]) and (got != before).sum() > 1000
