"""svr_demo --ao <radius>:<intensity> (include/svr_ambient.h).  Without a GPU: the flag's refusals, through the oracle, which
has no ambient pass.  On the GPU: an intensity of 0 gives the colour of a run without the flag, bit for bit, and an
intensity of 1 does not."""
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as g
import svr_testlib as T

W, H = 160, 90
RADIUS = "0.6"


run_demo = functools.partial(T.run_demo, width=W, height=H)


def test_ao_on_a_library_without_it_fails_loudly(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--ao", RADIUS + ":1")
    assert p.returncode != 0 and "--ao: the library has no ambient pass (include/svr_ambient.h)" in p.stdout
    assert not os.path.exists(str(tmp_path / "demo.color"))


@pytest.mark.parametrize("arg", ["0:1", "-0.5:1", "0.5", "0.5:", ":1", "0.5:-1", "nan:1", "0.5:nan", "inf:1", "0.5:inf", "0.5x:1", "0.5:1x", "x"])
def test_a_malformed_argument_is_refused(tmp_path, oracle, arg):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--ao", arg)
    assert p.returncode != 0 and "--ao: expected <radius > 0>:<intensity >= 0>" in p.stdout


def test_ao_needs_deferred_and_excludes_views_and_ranks(tmp_path, oracle):
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--ao", RADIUS + ":1")
    assert p.returncode != 0 and "--ao: needs --deferred 1" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--ao", RADIUS + ":1", "--views", "2")
    assert p.returncode != 0 and "--ao: not with --views" in p.stdout
    p = run_demo(oracle.path, str(tmp_path / "demo"), "--deferred", "1", "--ao", RADIUS + ":1", "--ranks", "2")
    assert p.returncode != 0 and "--ao: not with --ranks" in p.stdout


@pytest.mark.gpu
def test_demo_ao(tmp_path, hip):
    """the synthetic atrium through svr_demo --gltf (the default scene's two cubes are convex and apart: nothing occludes)"""
    pkg = g.load_package()
    IO = __import__(pkg.__name__ + ".gltf_io", fromlist=["write_glb"])
    glb = str(tmp_path / "atrium.glb")
    IO.write_glb(pkg.scenes.sponza_like(lod=8, tex_size=64), glb)
    (x, y, z), pitch, yaw = pkg.scenes.config3_camera()  # the view test_ambient_gpu.py's rendered G-buffer has creases in
    scene = ("--gltf", glb, "--camera", f"{x!r},{y!r},{z!r},{pitch!r},{yaw!r}", "--deferred", "1")
    colors = {}
    for name, extra in (("plain", ()), ("zero", ("--ao", RADIUS + ":0")), ("one", ("--ao", RADIUS + ":1"))):
        prefix = str(tmp_path / name)
        p = run_demo(hip.path, prefix, *scene, *extra, frames=1)
        assert p.returncode == 0, p.stdout
        colors[name] = np.fromfile(prefix + ".color", dtype=np.uint16).reshape(H, W, 4)
    assert np.array_equal(colors["zero"], colors["plain"]), "an intensity of 0 leaves every ambient term as it was"
    changed = np.any(colors["one"] != colors["plain"], axis=-1)
    assert changed.any(), f"an intensity of 1 darkens the creases ({int(changed.sum())} pixels differ)"
    assert not changed.all()
