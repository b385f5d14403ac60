"""Retained draw lists (include/svr_draw_list.h) on the MI355X: svr_draw_list must give what svr_draw_geometry gives on
the same arrays — frames bit for bit (and the oracle's frames), the device's draw records byte for byte, the stats —
through updates in flight, overflow replays, bands and interleaved rows; and it must refuse a list whose meshes are
gone instead of reading freed memory."""
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_full_frames", os.path.join(T.GOLDEN_DIR, "make_full_frames.py"))
MF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MF)

LIST_FUSED_MAX = 4096  # csrc/svr_device.h


def _as_objects(a):
    if a is None:
        return np.zeros(0, A.RENDER_OBJECT_DTYPE)
    return np.ascontiguousarray(a, dtype=A.RENDER_OBJECT_DTYPE)


def draw_via_list(self, scene, opaque, transparent=None):
    """Renderer.draw_geometry as a one-frame draw list: made, drawn and destroyed at once (stream-ordered)."""
    lst = self.create_draw_list(_as_objects(opaque), _as_objects(transparent))
    st = self.draw_list(scene, lst)
    lst.close()
    return st


def read_frame(r):
    return {"color": r.read_color(), "depth": r.read_depth(), "rgba8": r.read_color(as_rgba8=True), "stats": r.get_stats()}


HIP_STATS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "shaded_fragments",
             "binned_triangles", "bin_entries")
ORACLE_STATS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "binned_triangles")  # as test_parity_gpu


def assert_same(a, b, what, stats=HIP_STATS):
    T.assert_images_identical(a["color"], b["color"], what + " colour")
    T.assert_images_identical(a["depth"], b["depth"], what + " depth")
    T.assert_images_identical(a["rgba8"], b["rgba8"], what + " rgba8")
    for f in stats:
        assert getattr(a["stats"], f) == getattr(b["stats"], f), f"{what}: {f}"


# ---------------------------------------------------------------- frames
LIST_MAX_OBJECTS = 16384  # include/svr_draw_list.h
OVER_THE_LIST_CAP = {"soup_very_dense_split"}  # 36000 one-triangle objects


@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_scenario_frames(hip, oracle, name, monkeypatch):
    if name in OVER_THE_LIST_CAP:
        with monkeypatch.context() as m:
            m.setattr(A.Renderer, "draw_geometry", draw_via_list)
            with pytest.raises(A.SvrError) as ei:
                SC.SCENARIOS[name](hip)
        assert ei.value.code == -5 and str(LIST_MAX_OBJECTS) in str(ei.value)
        return
    want = SC.SCENARIOS[name](hip)
    ref = SC.SCENARIOS[name](oracle)
    with monkeypatch.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw_via_list)
        got = SC.SCENARIOS[name](hip)
    assert_same(got, want, name)
    assert_same(got, ref, name + " (oracle)", ORACLE_STATS)


@pytest.mark.parametrize("name", list(MF.FRAMES))
def test_full_frames_hash_to_the_oracle(hip, name):
    """configs[2], configs[3] and configs[4] uninstrumented (the hierarchical depth test is live)."""
    with open(MF.OUT) as f:
        d = json.load(f)[name]
    w, h, instanced = MF.FRAMES[name]
    kw = dict(camera=S.config5_camera(), instances=S.config5_instances()) if instanced else {}
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=MF.TEX, **kw)
    lst = r.create_draw_list(opaque, transparent)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    a = read_frame(r)
    r.clear_color((1, 1, 1, 1))
    r.draw_list(scene, lst)
    b = read_frame(r)
    lst.close()
    r.close()
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(b[key], a[key], f"{name} {key}")
        assert MF.sha(b[key]) == d[key], f"{name}: {key} digest"
    sa, sb = a["stats"], b["stats"]
    assert (sb.triangle_count, sb.drawcall_count, sb.culled_draws) == (sa.triangle_count, sa.drawcall_count, sa.culled_draws)
    assert sb.triangle_count == d["counters"]["triangle_count"] and sb.drawcall_count == d["counters"]["drawcall_count"]


# ---------------------------------------------------------------- records
def _sponza(hip, n_total=None, w=256, h=144):
    r, _, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    if n_total is not None:  # the same objects again (equal sort keys) up to n_total
        opaque = np.resize(opaque, n_total - len(transparent))
    return r, opaque, transparent


def _camera_path(seed, n, w, h):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pos = (float(rng.uniform(-25, 25)), float(rng.uniform(1, 12)), float(rng.uniform(-8, 8)))
        out.append(S.scene_data_struct(pos, float(rng.uniform(-0.6, 0.6)), float(rng.uniform(0, 6.283)), w, h))
    return out


def _scene_from_viewproj(vp):
    return A.scene_struct(GL.identity(), GL.identity(), vp, (0.1, 0.1, 0.1, 1), (0, 1, 0.5, 1), (1, 1, 1, 1))


def everything_culled():
    vp = np.zeros(16, np.float32)  # column-major: every point goes to (0, 0, -1, 1), in front of the depth range
    vp[14] = -1.0
    vp[15] = 1.0
    return _scene_from_viewproj(vp)


def nothing_culled():
    vp = np.zeros(16, np.float32)  # every point shrinks to the middle of the view volume: x, y ~ 0, z ~ 0.5
    vp[0] = vp[5] = vp[10] = 1e-4
    vp[14] = 0.5
    vp[15] = 1.0
    return _scene_from_viewproj(vp)


def records_and_stats(r, draw):
    r.clear_color((1, 1, 1, 1))
    draw()
    d, c = r.read_records()
    st = r.get_stats()
    return d, c, (st.drawcall_count, st.triangle_count, st.culled_draws), r.read_color(), r.read_depth()


def check_records(r, opaque, transparent, scenes, what):
    lst = r.create_draw_list(opaque, transparent)
    r.set_option(A.OPT_DEVICE_FLATTEN, 2)  # svr_draw_geometry on the host path: what it stages is the reference
    culled = []
    for k, scene in enumerate(scenes):
        want = records_and_stats(r, lambda: r.draw_geometry(scene, opaque, transparent))
        got = records_and_stats(r, lambda: r.draw_list(scene, lst))
        assert want[2] == got[2], f"{what} frame {k}: stats {got[2]} != {want[2]}"
        assert want[0].shape == got[0].shape and np.array_equal(want[0], got[0]), f"{what} frame {k}: DrawDesc records"
        assert want[1].shape == got[1].shape and np.array_equal(want[1], got[1]), f"{what} frame {k}: WaveChunk records"
        T.assert_images_identical(got[3], want[3], f"{what} frame {k} colour")
        T.assert_images_identical(got[4], want[4], f"{what} frame {k} depth")
        culled.append(want[2][2])
    lst.close()
    return culled


def test_records_on_a_camera_path(hip):
    r, opaque, transparent = _sponza(hip)
    culled = check_records(r, opaque, transparent, _camera_path(3, 6, 256, 144), "camera path")
    assert any(0 < c < len(opaque) for c in culled)
    r.close()


def test_records_everything_and_nothing_culled(hip):
    r, opaque, transparent = _sponza(hip)
    culled = check_records(r, opaque, transparent, [everything_culled(), nothing_culled()], "extremes")
    assert culled == [len(opaque), 0]
    r.close()


def test_records_equal_keys_and_no_transparent(hip):
    r, opaque, _ = _sponza(hip)
    twice = np.concatenate([opaque, opaque[::-1]])  # every key twice: the submission index decides
    check_records(r, twice, np.zeros(0, A.RENDER_OBJECT_DTYPE), _camera_path(5, 3, 256, 144), "equal keys")
    r.close()


@pytest.mark.parametrize("n_total", [LIST_FUSED_MAX, LIST_FUSED_MAX + 1])
def test_records_at_and_past_the_fused_cap(hip, n_total):
    r, opaque, transparent = _sponza(hip, n_total)
    assert len(opaque) + len(transparent) == n_total
    check_records(r, opaque, transparent, _camera_path(7, 2, 256, 144) + [nothing_culled()], f"{n_total} objects")
    r.close()


# ---------------------------------------------------------------- updates in flight
def run_updates(hip, queue_caps=None):
    import torch
    w, h = 256, 144
    r, opaque, transparent = _sponza(hip, w=w, h=h)
    ref, _, _ = _sponza(hip, w=w, h=h)
    scenes = _camera_path(11, 6, w, h)
    cur, tr = opaque.copy(), transparent.copy()
    hidden = 5
    cur["transform"][hidden, 13] -= 1000.0  # starts far below the floor: culled
    lst = r.create_draw_list(cur, tr)
    if queue_caps is not None:
        r.set_option(A.OPT_QUEUE_CAPS, queue_caps)
    targets = [(torch.empty((h, w, 4), dtype=torch.int16, device="cuda"), torch.empty((h, w), dtype=torch.float32, device="cuda"))
               for _ in scenes]
    states = []
    for k, scene in enumerate(scenes):
        if k == 1:  # a transform change
            upd = cur[10:12].copy()
            upd["transform"][:, 12] += 0.75
            cur[10:12] = upd
            lst.update(10, upd)
        if k == 3:  # the far object comes back into view
            cur[hidden] = opaque[hidden]
            lst.update(hidden, opaque[hidden:hidden + 1])
        if k == 4 and len(tr):  # an update in the transparent list
            upd = tr[:1].copy()
            upd["transform"][0, 13] += 0.5
            tr[:1] = upd
            lst.update(len(cur), upd)
        states.append((cur.copy(), tr.copy()))
        c, d = targets[k]
        r.bind_targets(c.data_ptr(), d.data_ptr())  # no fence: every frame in targets of its own, several in flight
        r.clear_color((1, 1, 1, 1))
        r.draw_list(scene, lst)
    r.sync()
    st = r.get_stats()
    r.bind_targets(None, None)
    for k, scene in enumerate(scenes):
        ref.clear_color((1, 1, 1, 1))
        ref.draw_geometry(scene, *states[k])
        c, d = targets[k]
        T.assert_images_identical(c.cpu().numpy().view(np.uint16), ref.read_color(), f"frame {k} colour")
        T.assert_images_identical(d.cpu().numpy(), ref.read_depth(), f"frame {k} depth")
    lst.close()
    r.close()
    ref.close()
    return st


def test_updates_between_unfenced_passes(hip):
    run_updates(hip)


def test_updates_under_overflow_replays(hip):
    st = run_updates(hip, queue_caps=64)
    assert st.replayed_passes > 0


# ---------------------------------------------------------------- invalidation and refusals
def _tiny(hip):
    rig = SC.Rig(hip, 32, 32)
    v = SC.make_vertices([(-1, -1, 0.5), (1, -1, 0.5), (1, 1, 0.5), (-1, 1, 0.5)])
    return rig, rig.r.upload_mesh(SC.QUAD_IDX, v), rig.r.upload_mesh(SC.QUAD_IDX, v)


def test_destroyed_mesh_invalidates_the_list(hip):
    rig, mesh, keep = _tiny(hip)
    mat = rig.material()
    lst = rig.r.create_draw_list(SC.objs([SC.render_object(mesh, mat, 0, 6), SC.render_object(keep, mat, 0, 6)]))
    scene = SC.identity_scene()
    rig.r.draw_list(scene, lst)
    rig.r.destroy_mesh(mesh)
    with pytest.raises(A.SvrError) as ei:
        rig.r.draw_list(scene, lst)
    assert ei.value.code == -1 and "mesh" in str(ei.value)
    lst.update(0, SC.objs([SC.render_object(keep, mat, 0, 6)]))  # repaired
    rig.r.draw_list(scene, lst)
    rig.r.sync()
    lst.close()
    rig.finish()


def test_material_pass_rules_and_refusals(hip):
    rig, mesh, _ = _tiny(hip)
    mo, mt = rig.material(), rig.material(transparent=True)
    with pytest.raises(A.SvrError) as ei:  # a Transparent material in the opaque list
        rig.r.create_draw_list(SC.objs([SC.render_object(mesh, mt, 0, 6)]))
    assert ei.value.code == -1 and "svr_create_draw_list" in str(ei.value)
    lst = rig.r.create_draw_list(SC.objs([SC.render_object(mesh, mo, 0, 6)]), SC.objs([SC.render_object(mesh, mt, 0, 6)]))
    with pytest.raises(A.SvrError) as ei:  # a non-Transparent material into the transparent list
        lst.update(1, SC.objs([SC.render_object(mesh, mo, 0, 6)]))
    assert ei.value.code == -1
    with pytest.raises(A.SvrError) as ei:  # n beyond the list
        lst.update(1, SC.objs([SC.render_object(mesh, mt, 0, 6)] * 2))
    assert ei.value.code == -1
    with pytest.raises(A.SvrError) as ei:  # index range outside the mesh
        lst.update(0, SC.objs([SC.render_object(mesh, mo, 0, 9)]))
    assert ei.value.code == -1
    with pytest.raises(A.SvrError) as ei:  # null list
        rig.r.draw_list(SC.identity_scene(), 0)
    assert ei.value.code == -4
    handle = lst.handle
    lst.close()
    with pytest.raises(A.SvrError) as ei:  # destroyed list
        rig.r.draw_list(SC.identity_scene(), handle)
    assert ei.value.code == -4
    rig.finish()


def test_colour_factors_come_from_the_material_table(hip):
    rig, mesh, _ = _tiny(hip)
    red, blue = rig.material((1, 0, 0, 1)), rig.material((0, 0, 1, 1))
    lst = rig.r.create_draw_list(SC.objs([SC.render_object(mesh, red, 0, 6)]))
    rig.r.clear_color((1, 1, 1, 1))
    rig.r.draw_list(SC.identity_scene(), lst)
    a = rig.r.read_color(as_rgba8=True)
    lst.update(0, SC.objs([SC.render_object(mesh, blue, 0, 6)]))
    rig.r.clear_color((1, 1, 1, 1))
    rig.r.draw_list(SC.identity_scene(), lst)
    b = rig.r.read_color(as_rgba8=True)
    assert a[16, 16, 0] > 0 and a[16, 16, 2] == 0 and b[16, 16, 0] == 0 and b[16, 16, 2] > 0
    lst.close()
    rig.finish()


# ---------------------------------------------------------------- bands and interleaved rows
@pytest.mark.parametrize("mode,n", [("bands", 2), ("bands", 3), ("interleave", 2), ("interleave", 3)])
def test_contexts_compose_the_frame(hip, mode, n):
    w, h = 320, 200
    full, opaque, transparent = _sponza(hip, w=w, h=h)
    scene = S.scene_data_struct(*S.config3_camera(), w, h)
    full.clear_color((1, 1, 1, 1))
    full.draw_geometry(scene, opaque, transparent)
    want_c, want_d = full.read_color(), full.read_depth()
    full.close()
    color, depth = np.zeros_like(want_c), np.zeros_like(want_d)
    for k in range(n):
        r, _, _ = _sponza(hip, w=w, h=h)
        lst = r.create_draw_list(opaque, transparent)
        if mode == "bands":
            # even rows: a band that starts on an odd row shifts the 2x2 quads the derivatives are taken over
            y0, y1 = (k * h // n) & ~1, ((k + 1) * h // n) & ~1 if k + 1 < n else h
            r.set_scissor(0, y0, w, y1 - y0)
            rows = np.arange(y0, y1)
        else:
            r.set_row_interleave(n, k)
            rows = np.array([y for y in range(h) if (y // 32) % n == k])
        r.clear_color((1, 1, 1, 1))
        r.draw_list(scene, lst)
        c, d = r.read_color(), r.read_depth()
        color[rows], depth[rows] = c[rows], d[rows]
        lst.close()
        r.close()
    T.assert_images_identical(color, want_c, f"{mode} x{n} colour")
    T.assert_images_identical(depth, want_d, f"{mode} x{n} depth")


def test_context_without_tile_rows_draws_nothing(hip):
    r, opaque, transparent = _sponza(hip, w=96, h=40)
    r.set_row_interleave(3, 2)  # two tile rows: offset 2 owns none
    lst = r.create_draw_list(opaque, transparent)
    st = r.draw_list(S.scene_data_struct(*S.config3_camera(), 96, 40), lst)
    assert st.drawcall_count == 0
    lst.close()
    r.close()
