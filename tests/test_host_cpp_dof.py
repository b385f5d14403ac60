"""svr_demo --deferred 1 --dof <focus_distance>:<blur_scale>[:<max_radius>]: the C++ engine runs the depth of field pass
(include/svr_dof.h) behind the deferred frame's transparent objects.  On the GPU the .color dump must be what the Python
path leaves when it runs the same pass (the dumped <prefix>.dof) over the targets of the run without the flag; the oracle
has no such pass, so on the CPU the flag must fail loudly, as must a malformed one.  The caller-side helpers of
host/svr_math.h are held to glmath.py's bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g
import dof_ref as DR
import native_ref as N
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
GL = pkg.glmath
HOST_DIR = os.path.join(g.PKG_DIR, "host")
W, H = 96, 54


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_dof_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--dof", "8:6:12")
    assert p.returncode != 0 and "--dof: the library has no depth of field pass (include/svr_dof.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["8", "8:", "8:6:", "8:6:17", "8:6:-1", "8:6:12x", "0:6", "-1:6", "8:-2", "a:b", ":6", "inf:6", "8:nan"])
def test_a_malformed_dof_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--dof", arg)
    assert p.returncode != 0 and "--dof: expected <focus_distance > 0>:<blur_scale >= 0>[:<max_radius in 0..16>]" in p.stdout


def test_dof_needs_the_deferred_frame_and_excludes_views_and_ranks(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--dof", "8:6")
    assert p.returncode != 0 and "--dof: needs --deferred 1" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--dof", "8:6", "--views", "2")
    assert p.returncode != 0 and "--dof: not with --views" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--dof", "8:6", "--ranks", "2")
    assert p.returncode != 0 and "--dof: not with --ranks" in p.stdout


HELPERS_SRC = r'''
#include <cstdio>
#include <cstring>
#include "svr_math.h"
int main() {
  float v[8];
  while (std::fread(v, 4, 8, stdin) == 8) {
    svrm::mat4 proj = svrm::perspective(v[0], v[1], 10000.f, 0.1f);
    proj.m[1][1] *= -1.f;
    float out[3];
    svrm::dof_depth_terms(proj, &out[0], &out[1]);
    out[2] = svrm::dof_blur_scale(v[2], v[3], v[4], v[5], v[6]);
    std::fwrite(out, 4, 3, stdout);
  }
  return 0;
}
'''


def test_host_helpers_match_glmath(tmp_path):
    src = tmp_path / "helpers.cpp"
    src.write_text(HELPERS_SRC)
    exe = N.build(str(src), include=(HOST_DIR,))
    rng = np.random.default_rng(3)
    rows = np.stack([rng.uniform(0.3, 2.0, 64), rng.uniform(0.5, 2.5, 64), rng.uniform(0.01, 0.2, 64), rng.uniform(1.0, 22.0, 64),
                     rng.uniform(0.3, 50.0, 64), rng.uniform(0.01, 0.05, 64), rng.integers(1, 4321, 64), np.zeros(64)], axis=1).astype(np.float32)
    out = subprocess.run([str(exe)], input=rows.tobytes(), check=True, stdout=subprocess.PIPE).stdout
    got = np.frombuffer(out, np.float32).reshape(64, 3)
    for row, res in zip(rows, got):
        proj = GL.perspective_rh_zo(row[0], row[1], 10000.0, 0.1)
        proj[1][1] *= np.float32(-1)
        want = [*GL.dof_depth_terms(proj), GL.dof_blur_scale(*row[2:7])]
        assert np.array_equal(np.array(want, np.float32).view(np.uint32), res.view(np.uint32)), row


@pytest.mark.gpu
def test_deferred_dof_dump_is_the_python_path_over_the_plain_dump(tmp_path, hip):
    torch = pytest.importorskip("torch")
    plain, blurred = str(tmp_path / "plain"), str(tmp_path / "blurred")
    p = run_demo(hip.path, plain, "--deferred", "1")
    assert p.returncode == 0, p.stdout
    q = run_demo(hip.path, blurred, "--deferred", "1", "--dof", "8:6:12")
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(H, W, 4)
    depth = np.fromfile(f"{plain}.depth", dtype=np.float32).reshape(H, W)
    got = np.fromfile(f"{blurred}.color", dtype=np.uint16).reshape(H, W, 4)
    raw = open(f"{blurred}.dof", "rb").read()
    assert len(raw) == C.sizeof(A.SvrDofPass)
    dp = A.SvrDofPass.from_buffer_copy(raw)
    assert (dp.focus_distance, dp.blur_scale, dp.max_radius) == (8.0, 6.0, 12.0)
    proj = GL.perspective_rh_zo(GL.radians(70.0), np.float32(W) / np.float32(H), 10000.0, 0.1)
    assert (np.float32(dp.inv_z_scale), np.float32(dp.inv_z_bias)) == GL.dof_depth_terms(proj), "the terms of the scene's projection"
    # the Python path: the same pass over the plain run's targets, in caller tensors
    color_t = torch.from_numpy(before.view(np.int32).reshape(H, W, 2).copy()).cuda()
    depth_t = torch.from_numpy(depth.copy()).cuda()
    torch.cuda.synchronize()
    r = hip.create(W, H)
    r.bind_targets(color_t.data_ptr(), depth_t.data_ptr())
    hip.check(hip.lib.svr_dof_pass(r.h, C.byref(dp)))
    r.sync()
    want = color_t.cpu().numpy().view(np.uint16).reshape(H, W, 4)
    r.close()
    assert not np.array_equal(want, before)
    assert np.array_equal(got, want)
    # ... which is the restatement's
    ref = DR.run_ref(before, depth, (dp.inv_z_scale, dp.inv_z_bias), dp.focus_distance, dp.blur_scale, dp.max_radius)["color"]
    assert np.array_equal(got, ref)
    for k in ("depth", "opaque", "transparent", "scene"):
        assert np.array_equal(np.fromfile(f"{plain}.{k}", dtype=np.uint8), np.fromfile(f"{blurred}.{k}", dtype=np.uint8)), k
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8), np.fromfile(f"{blurred}.swapchain", dtype=np.uint8))
