"""svr_demo --deferred 1 --fog <density>:<falloff>[:<g>]: the C++ engine runs the fog pass (include/svr_fog.h) behind the
deferred frame's transparent objects.  On the GPU the .color dump must be what the Python path leaves when it runs the same
pass (the dumped <prefix>.fog) over the targets of the run without the flag; the oracle has no fog pass, so on the CPU the
flag must fail loudly, as must a malformed one."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as g
import fog_ref as FR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
W, H = 96, 54


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_fog_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--fog", "0.05:0.1")
    assert p.returncode != 0 and "--fog: the library has no fog pass (include/svr_fog.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["0.05", "0.05:", "0.05:0.1:", "0.05:0.1:1.0", "0.05:0.1:0.5x", "-1:0.1", "0.05:-2", "a:b", ":0.1"])
def test_a_malformed_fog_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--fog", arg)
    assert p.returncode != 0 and "--fog: expected <density >= 0>:<falloff >= 0>[:<g in (-1, 1)>]" in p.stdout


def test_fog_needs_the_deferred_frame_and_excludes_views(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--fog", "0.05:0.1")
    assert p.returncode != 0 and "--fog: needs --deferred 1" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--fog", "0.05:0.1", "--views", "2")
    assert p.returncode != 0 and "--fog: not with --views" in p.stdout


@pytest.mark.gpu
def test_deferred_fog_dump_is_the_python_path_over_the_plain_dump(tmp_path, hip):
    torch = pytest.importorskip("torch")
    plain, fogged = str(tmp_path / "plain"), str(tmp_path / "fogged")
    p = run_demo(hip.path, plain, "--deferred", "1")
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, fogged, "--deferred", "1", "--fog", "0.02:0.05:0.6")
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(H, W, 4)
    depth = np.fromfile(f"{plain}.depth", dtype=np.float32).reshape(H, W)
    got = np.fromfile(f"{fogged}.color", dtype=np.uint16).reshape(H, W, 4)
    raw = open(f"{fogged}.fog", "rb").read()
    assert len(raw) == C.sizeof(A.SvrFogPass)
    fp = A.SvrFogPass.from_buffer_copy(raw)
    assert (fp.density, fp.height_falloff, fp.anisotropy) == tuple(float(np.float32(v)) for v in (0.02, 0.05, 0.6))
    assert fp.steps == 16 and fp.frame_index == 0 and not fp.shadow_depth
    # the Python path: the same pass over the plain run's targets, in caller tensors
    color_t = torch.from_numpy(before.view(np.int32).reshape(H, W, 2).copy()).cuda()
    depth_t = torch.from_numpy(depth.copy()).cuda()
    torch.cuda.synchronize()
    r = hip.create(W, H)
    r.bind_targets(color_t.data_ptr(), depth_t.data_ptr())
    hip.check(hip.lib.svr_fog_pass(r.h, C.byref(fp)))
    r.sync()
    want = color_t.cpu().numpy().view(np.uint16).reshape(H, W, 4)
    r.close()
    assert not np.array_equal(want, before)
    assert np.array_equal(got, want)
    # ... which is the restatement's
    ref = FR.run_ref(before, depth, np.array(fp.inv_viewproj, np.float32), np.array(fp.camera_position, np.float32), density=fp.density,
                     height_falloff=fp.height_falloff, height_base=fp.height_base, max_distance=fp.max_distance, steps=fp.steps,
                     fog_color=tuple(fp.fog_color), sun_dir=tuple(fp.sunlight_direction), sun_color=tuple(fp.sun_color),
                     anisotropy=fp.anisotropy, edge_sharpness=fp.edge_sharpness, frame_index=fp.frame_index)["color"]
    assert np.array_equal(got, ref)
    for k in ("depth", "opaque", "transparent", "scene"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{fogged}.{k}", dtype=np.uint8)), k
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8), np.fromfile(f"{fogged}.swapchain", dtype=np.uint8))
