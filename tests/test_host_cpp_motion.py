"""svr_demo --deferred 1 --motion-blur <shutter>:<yaw_degrees>[:<max_blur>]: the C++ engine runs the camera motion blur
pass (include/svr_motion.h) behind the deferred frame's transparent objects.  On the GPU the .color dump must be what the
Python path leaves when it runs the same pass (the dumped <prefix>.motion) over the targets of the run without the flag;
the oracle has no such pass, so on the CPU the flag must fail loudly, as must a malformed or misused one."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as g
import motion_ref as MR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
GL = pkg.glmath
W, H = 96, 54

run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_motion_blur_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--motion-blur", "1:5:12")
    assert p.returncode != 0 and "--motion-blur: the library has no motion blur pass (include/svr_motion.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["1", "1:", "1:5:", "1:5:17", "1:5:-1", "1:5:12x", "-1:5", "a:b", ":5", "inf:5", "1:nan", "1:inf", "nan:5"])
def test_a_malformed_motion_blur_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--motion-blur", arg)
    assert p.returncode != 0 and "--motion-blur: expected <shutter >= 0>:<yaw_degrees>[:<max_blur in 0..16>]" in p.stdout


def test_motion_blur_needs_the_deferred_frame_and_excludes_views_and_ranks(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--motion-blur", "1:5")
    assert p.returncode != 0 and "--motion-blur: needs --deferred 1" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--motion-blur", "1:5", "--views", "2")
    assert p.returncode != 0 and "--motion-blur: not with --views" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--motion-blur", "1:5", "--ranks", "2")
    assert p.returncode != 0 and "--motion-blur: not with --ranks" in p.stdout


@pytest.mark.gpu
def test_deferred_motion_blur_dump_is_the_python_path_over_the_plain_dump(tmp_path, hip):
    torch = pytest.importorskip("torch")
    plain, blurred = str(tmp_path / "plain"), str(tmp_path / "blurred")
    p = run_demo(hip.path, plain, "--deferred", "1")
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, blurred, "--deferred", "1", "--motion-blur", "1:5:12")
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(H, W, 4)
    depth = np.fromfile(f"{plain}.depth", dtype=np.float32).reshape(H, W)
    got = np.fromfile(f"{blurred}.color", dtype=np.uint16).reshape(H, W, 4)
    raw = open(f"{blurred}.motion", "rb").read()
    assert len(raw) == C.sizeof(A.SvrMotionBlurPass) == 72
    mp = A.SvrMotionBlurPass.from_buffer_copy(raw)
    assert (mp.shutter, mp.max_blur) == (1.0, 12.0)
    rp = np.array(mp.reproject, np.float32).reshape(4, 4)
    assert np.isfinite(rp).all() and not np.allclose(rp, GL.identity()), "the previous camera is this frame's turned by 5 degrees"
    # the Python path: the same pass over the plain run's targets, in caller tensors
    color_t = torch.from_numpy(before.view(np.int32).reshape(H, W, 2).copy()).cuda()
    depth_t = torch.from_numpy(depth.copy()).cuda()
    torch.cuda.synchronize()
    r = hip.create(W, H)
    r.bind_targets(color_t.data_ptr(), depth_t.data_ptr())
    hip.check(hip.lib.svr_motion_blur_pass(r.h, C.byref(mp)))
    r.sync()
    want = color_t.cpu().numpy().view(np.uint16).reshape(H, W, 4)
    r.close()
    assert not np.array_equal(want, before)
    assert np.array_equal(got, want)
    # ... which is the restatement's
    ref = MR.run_ref(before, depth, rp, mp.shutter, mp.max_blur)
    assert np.array_equal(got, ref["color"])
    v = MR.floats(ref["v"])
    assert np.hypot(v[..., 0], v[..., 1]).max() > 1.0, "a turn of 5 degrees moves the frame"
    for k in ("depth", "opaque", "transparent", "scene"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{blurred}.{k}", dtype=np.uint8)), k
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8), np.fromfile(f"{blurred}.swapchain", dtype=np.uint8))
