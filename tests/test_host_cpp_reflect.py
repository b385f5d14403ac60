"""svr_demo --deferred 1 --reflect <intensity>:<max_distance>[:<steps>]: the C++ engine runs the reflection pass
(include/svr_reflect.h) behind the deferred frame's transparent objects.  On the GPU the .color dump must be what the Python
path leaves when it runs the same pass (the dumped <prefix>.reflect) over the targets of the run without the flag and the
dumped G-buffer planes; the oracle has no reflection pass, so on the CPU the flag must fail loudly, as must a malformed one.
The GPU run takes the synthetic atrium through svr_demo --gltf: the default scene's two cubes have no floor under them and
reflect nothing."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as g
import reflect_ref as RR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
W, H = 160, 90


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_reflect_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--reflect", "1:20")
    assert p.returncode != 0 and "--reflect: the library has no reflection pass (include/svr_reflect.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["1", "1:", "1:20:", "1:20:0", "1:20:65", "1:20:-3", "1:20:8x", "-1:20", "1:0", "1:-2", "a:b", ":20"])
def test_a_malformed_reflect_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--reflect", arg)
    assert p.returncode != 0 and "--reflect: expected <intensity >= 0>:<max_distance > 0>[:<steps in 1..64>]" in p.stdout


def test_reflect_needs_the_deferred_frame_and_excludes_views(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--reflect", "1:20")
    assert p.returncode != 0 and "--reflect: needs --deferred 1" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--reflect", "1:20", "--views", "2")
    assert p.returncode != 0 and "--reflect: not with --views" in p.stdout


@pytest.mark.gpu
def test_deferred_reflect_dump_is_the_python_path_over_the_plain_dump(tmp_path, hip):
    torch = pytest.importorskip("torch")
    IO = __import__(pkg.__name__ + ".gltf_io", fromlist=["write_glb"])
    glb = str(tmp_path / "atrium.glb")
    IO.write_glb(pkg.scenes.sponza_like(lod=8, tex_size=64), glb)
    (x, y, z), pitch, yaw = pkg.scenes.config3_camera()  # the view test_reflect_gpu.py's sponza frames reflect in
    scene = ("--gltf", glb, "--camera", f"{x!r},{y!r},{z!r},{pitch!r},{yaw!r}", "--deferred", "1")
    plain, reflected = str(tmp_path / "plain"), str(tmp_path / "reflected")
    p = run_demo(hip.path, plain, *scene, frames=1)
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, reflected, *scene, "--reflect", "4:12:24", frames=1)
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(H, W, 4)
    depth = np.fromfile(f"{plain}.depth", dtype=np.float32).reshape(H, W)
    normal = np.fromfile(f"{reflected}.normal", dtype=np.float32).reshape(H, W, 4)
    albedo = np.fromfile(f"{reflected}.albedo", dtype=np.float32).reshape(H, W, 4)
    got = np.fromfile(f"{reflected}.color", dtype=np.uint16).reshape(H, W, 4)
    raw = open(f"{reflected}.reflect", "rb").read()
    assert len(raw) == C.sizeof(A.SvrReflectPass)
    rp = A.SvrReflectPass.from_buffer_copy(raw)
    assert (rp.intensity, rp.max_distance, rp.steps, rp.refine, rp.resolve, rp.frame_index) == (4.0, 12.0, 24, 4, 1, 0)
    assert tuple(rp.viewproj) == tuple(A.SvrSceneData.from_buffer_copy(open(f"{reflected}.scene", "rb").read()).viewproj)
    # the Python path: the same pass over the plain run's targets and the dumped planes, in caller tensors
    color_t = torch.from_numpy(before.view(np.int32).reshape(H, W, 2).copy()).cuda()
    planes = [torch.from_numpy(a.copy()).cuda() for a in (depth, normal, albedo)]
    torch.cuda.synchronize()
    r = hip.create(W, H)
    r.bind_targets(color_t.data_ptr(), planes[0].data_ptr())
    r.bind_attribute_target(A.ATTR_NORMAL, planes[1].data_ptr())
    r.bind_attribute_target(A.ATTR_ALBEDO, planes[2].data_ptr())
    hip.check(hip.lib.svr_reflect_pass(r.h, C.byref(rp)))
    r.sync()
    want = color_t.cpu().numpy().view(np.uint16).reshape(H, W, 4)
    r.close()
    assert not np.array_equal(want, before)
    assert np.array_equal(got, want)
    # ... which is the restatement's
    ref = RR.run_ref(dict(color=before, depth=depth, normal=normal, albedo=albedo), np.array(rp.viewproj, np.float32), np.array(rp.inv_viewproj, np.float32),
                     np.array(rp.camera_position, np.float32), rp.inv_z_scale, rp.inv_z_bias, max_distance=rp.max_distance, steps=rp.steps,
                     refine=rp.refine, thickness=rp.thickness, f0=rp.f0, intensity=rp.intensity, distance_fade=rp.distance_fade,
                     edge_width=rp.edge_width, resolve=rp.resolve, depth_tolerance=rp.depth_tolerance, frame_index=rp.frame_index)
    assert (ref["hit"][..., 0] >= 0).sum() > 0
    assert np.array_equal(got, ref["color"])
    for k in ("depth", "opaque", "transparent", "scene"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{reflected}.{k}", dtype=np.uint8)), k
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8), np.fromfile(f"{reflected}.swapchain", dtype=np.uint8))
