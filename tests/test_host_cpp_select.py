"""svr_demo --select X,Y: the C++ engine reads the ID target (include/svr_ids.h) after its last frame and names the
RenderObject, mesh, surface and triangle that won pixel (X, Y).  It must name what the Python binding's pick gives for
the same lists and camera, immediate and retained.  The oracle has no ID target: there the flag fails loudly."""
import re

import numpy as np
import pytest

import __graft_entry__ as g
import svr_testlib as T
import test_host_cpp as HC

pkg = g.load_package()
A = pkg.abi
W, H = HC.W, HC.H


def select(lib_path, prefix, x, y, retained=False):
    return T.run_demo(lib_path, prefix, "--retained", "1" if retained else "0", "--select", f"{x},{y}", width=W, height=H)


def test_select_on_a_library_without_ids_fails_loudly(tmp_path, oracle):
    p = select(oracle.path, str(tmp_path / "demo"), 1, 1)
    assert p.returncode != 0 and "no ID target" in p.stdout


def python_ids(hip, demo_prefix, monkeypatch):
    """the lists and scene the demo dumped, drawn through the Python binding with IDs on"""
    opaque = np.fromfile(demo_prefix + ".opaque", dtype=A.RENDER_OBJECT_DTYPE)
    transparent = np.fromfile(demo_prefix + ".transparent", dtype=A.RENDER_OBJECT_DTYPE)
    scene = np.fromfile(demo_prefix + ".scene", dtype=np.float32)
    orig_draw, orig_finish = A.Renderer.draw_geometry, T._finish

    def draw(self, *a, **k):
        self.enable_ids()
        return orig_draw(self, *a, **k)

    def finish(r, stats=None):
        out = orig_finish(r, stats)
        out["ids"] = r.read_ids()
        out["pick"] = {xy: r.pick(*xy) for xy in PIXELS}
        return out

    with monkeypatch.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        m.setattr(T, "_finish", finish)
        return HC.python_side(hip, objects=(opaque, transparent), scene_floats=scene)


PIXELS = [(0, 0), (40, 45), (80, 45), (100, 30), (120, 60), (159, 89)]


@pytest.mark.gpu
@pytest.mark.parametrize("retained", [False, True])
def test_select_names_what_python_picks(tmp_path, hip, monkeypatch, retained):
    prefix = str(tmp_path / "demo")
    first = select(hip.path, prefix, 0, 0, retained)
    assert first.returncode == 0, first.stdout
    py = python_ids(hip, prefix, monkeypatch)
    ids = py["ids"]
    assert len(np.unique(ids[..., 0])) == 3  # background and both opaque objects are on screen
    # one pixel of each object, where it first appears in row-major order, besides the fixed ones
    pixels = list(PIXELS) + [(int(np.argwhere(ids[..., 0] == o)[0][1]), int(np.argwhere(ids[..., 0] == o)[0][0])) for o in (1, 2)]
    opaque = np.fromfile(prefix + ".opaque", dtype=A.RENDER_OBJECT_DTYPE)
    for x, y in pixels:
        p = select(hip.path, prefix, x, y, retained)
        assert p.returncode == 0, p.stdout
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("select ")]
        assert len(line) == 1, p.stdout
        o, prim = int(ids[y, x, 0]), int(ids[y, x, 1])
        if (x, y) in py["pick"]:
            assert py["pick"][(x, y)] == (None if o == 0 else (o, prim))
        if o == 0:
            assert line[0] == f"select {x} {y} none"
            continue
        m = re.fullmatch(rf"select {x} {y} object (\d+) mesh (\S+) surface (\d+) primitive (\d+)", line[0])
        assert m, line[0]
        assert (int(m[1]), int(m[4])) == (o, prim)
        # the demo's scene (test_host_cpp.python_side): one mesh "cubes" of two surfaces drawn by two nodes; surface 0
        # has the opaque material, surface 1 the transparent one
        assert m[2] == "cubes" and int(m[3]) == 0 and opaque[o - 1]["first_index"] == 0
