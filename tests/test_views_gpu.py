"""Multiview passes (include/svr_views.h) on the MI355X.

Every layer of a multiview pass must be, bit for bit, what a single-view pass over that layer's scene gives: against the
CPU oracle on the atrium's six cube faces, and against K single passes of the HIP library itself on the edge-case
scenarios (colour, depth, IDs and summed stats).  The layered targets are torch tensors [K, H, W, C]."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T
from test_ids_gpu import TUNE_NO_SPLIT

pkg = g.load_package()
A, S, GM = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TUNE_NO_HIZ, TUNE_HIZ = 32, 64  # SVR_OPT_TUNING bits (csrc/svr_device.h)
SUM_STATS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "shaded_fragments",
             "binned_triangles", "bin_entries")
f32 = np.float32


def _layers(r, n, init_color=None, ids=False):
    """device targets of n layers of the renderer's extent; colour from init_color (one layer, raw texels), depth and
    IDs filled with garbage the pass must overwrite"""
    h, w = r.height, r.width
    cdt = np.uint16 if r.color_format == A.COLOR_RGBA16F else np.uint8
    if init_color is None:
        init_color = np.random.default_rng(5).integers(0, 1 << 8 * cdt().itemsize, (h, w, 4)).astype(cdt)
    color = torch.from_numpy(np.broadcast_to(init_color.view(cdt).reshape(h, w, 4), (n, h, w, 4)).copy()).cuda()
    depth = torch.full((n, h, w), 0.5, dtype=torch.float32, device="cuda")
    idt = torch.full((n, h, w, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if ids else None
    torch.cuda.synchronize()
    return color, depth, idt


def _read(r, color, depth, idt):
    r.sync()
    torch.cuda.synchronize()
    out = {"color": color.cpu().numpy(), "depth": depth.cpu().numpy()}
    if idt is not None:
        out["ids"] = idt.cpu().numpy().view(np.uint32)
    return out


def _ptr(t):
    return None if t is None else t.data_ptr()


def _single(r, scene, opaque, transparent, init_color, ids=False):
    """one single-view pass into fresh targets that start as init_color; its layer and stats"""
    color, depth, idt = _layers(r, 1, init_color, ids)
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    if ids:
        r.bind_id_target(idt.data_ptr())
    r.draw_geometry(scene, opaque, transparent)
    st = r.get_stats()
    out = _read(r, color, depth, idt)
    r.bind_targets(None, None)
    if ids:
        r.bind_id_target(None)
    return {k: v[0] for k, v in out.items()}, st


def _views(r, scenes, opaque, transparent, init_color, ids=False, lst=None, clear=None):
    color, depth, idt = _layers(r, len(scenes), init_color, ids)
    if lst is None:
        r.draw_views(scenes, color.data_ptr(), depth.data_ptr(), opaque, transparent, ids_ptr=_ptr(idt), clear_rgba=clear)
    else:
        r.draw_list_views(scenes, lst, color.data_ptr(), depth.data_ptr(), ids_ptr=_ptr(idt), clear_rgba=clear)
    st = r.get_stats()
    return _read(r, color, depth, idt), st


def _assert_layer(got, k, want, what):
    for key in want:
        T.assert_images_identical(got[key][k], want[key], f"{what} layer {k} {key}")


def clip_transformed(scene, k):
    """the scene seen through a per-view clip-space transform (scale, shift and a little rotation of x/y)"""
    a = 0.07 * k
    s = 1.0 - 0.04 * k
    m = np.eye(4, dtype=np.float64)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = s * np.cos(a), -s * np.sin(a), s * np.sin(a), s * np.cos(a)
    m[0, 3], m[1, 3] = 0.06 * np.sin(1.7 * k), -0.05 * np.cos(1.3 * k)
    vp = np.array(scene.viewproj, dtype=np.float64).reshape(4, 4).T  # column-major -> row-major
    nvp = (m @ vp).astype(f32)
    out = A.SvrSceneData()
    ctypes.memmove(ctypes.addressof(out), ctypes.addressof(scene), ctypes.sizeof(out))
    for i, v in enumerate(nvp.T.reshape(16)):
        out.viewproj[i] = float(v)
    return out


def cube_scenes(w, h, pos=(0.0, 2.0, 0.0)):
    faces = [(0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (89.0, 0.0), (-89.0, 0.0)]
    out = []
    for pitch, yaw in faces:
        view = GM.camera_view(pos, f32(GM.radians(pitch)), f32(GM.radians(yaw)))
        _, _, _, amb, sun_dir, sun_col = GM.scene_data(view, w, h)
        proj = GM.perspective_rh_zo(GM.radians(90.0), f32(w) / f32(h), 10000.0, 0.1)
        proj[1][1] *= f32(-1)
        out.append((view, proj, GM.matmul(proj, view), amb, sun_dir, sun_col))
    return out


# ---------------------------------------------------------------- against the oracle
def test_cube_faces_match_the_oracle(hip, oracle):
    w, h = 256, 144
    faces = cube_scenes(w, h)
    r, _, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    white = np.full((h, w, 4), 0x3c00, np.uint16)  # RGBA16F 1.0
    got, st = _views(r, [A.scene_struct(*f) for f in faces], opaque, transparent, white)
    r.close()
    total = 0
    for k, f in enumerate(faces):
        o, scene, op, tr = T.setup_sponza(oracle, w, h, lod=8, tex_size=64)
        o.clear_color((1, 1, 1, 1))
        ost = o.draw_geometry(A.scene_struct(*f), op, tr)
        want = T._finish(o)
        o.close()
        _assert_layer(got, k, {"color": want["color"].view(np.uint16).reshape(h, w, 4), "depth": want["depth"]}, f"face {k}")
        total += ost.drawcall_count
    assert st.drawcall_count == total


# ---------------------------------------------------------------- against K single passes
SCEN = sorted(SC.SCENARIOS)
KS = (1, 2, 6, 16)


def _capture(lib, name, mp):
    """the scenario's renderer, scene, objects and colour just before its draw (the pass itself is not run)"""
    box = {}
    orig_finish = T._finish

    def draw(self, scene, opaque, transparent=None):
        box.update(r=self, scene=scene, opaque=opaque, transparent=transparent)
        raise StopIteration

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        m.setattr(T, "_finish", orig_finish)
        try:
            SC.SCENARIOS[name](lib)
        except StopIteration:
            pass
    return box


def _init_color(r):
    raw = r.read_color()  # flushes a deferred clear: what the scenario's pass would have loaded
    cdt = np.uint16 if r.color_format == A.COLOR_RGBA16F else np.uint8
    return raw.view(cdt).reshape(r.height, r.width, 4).copy()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCEN)
def test_layers_match_single_passes(hip, name, k, monkeypatch):
    box = _capture(hip, name, monkeypatch)
    if "r" not in box:
        pytest.fail(f"{name}: no draw_geometry call")
    r = box["r"]
    r.set_scissor(0, 0, r.width, r.height)  # a narrowed scissor has no multiview form: both sides draw the whole target
    init = _init_color(r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    scenes = [clip_transformed(box["scene"], i) for i in range(k)]
    got, st = _views(r, scenes, box["opaque"], box["transparent"], init, ids=True)
    sums = {f: 0 for f in SUM_STATS}
    wants = []
    for i, sc in enumerate(scenes):
        want, wst = _single(r, sc, box["opaque"], box["transparent"], init, ids=True)
        wants.append(want)
        _assert_layer(got, i, want, f"{name} K={k}")
        for f in SUM_STATS:
            sums[f] += getattr(wst, f)
    for f in SUM_STATS:
        assert getattr(st, f) == sums[f], f"{name}: {f}"
    if k == 2:  # the instances without the quarter path (tile_mv_kernel, tile_mv_ids_kernel <.., SPLIT = false>): the same layers
        r.set_option(A.OPT_TUNING, TUNE_NO_SPLIT)
        for ids in (True, False):
            for instr in (1, 0):
                r.set_option(A.OPT_COUNT_FRAGMENTS, instr)
                got, _ = _views(r, scenes, box["opaque"], box["transparent"], init, ids=ids)
                for i, want in enumerate(wants):
                    _assert_layer(got, i, {key: v for key, v in want.items() if ids or key != "ids"},
                                  f"{name} K={k} no split ids={ids} instr={instr}")
    r.close()


@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8])
@pytest.mark.parametrize("k", KS)
def test_atrium_odd_height(hip, fmt, k):
    """96 x 54: every layer's last tile row is partial"""
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64, color_format=fmt)
    init = _layers(r, 1)[0].cpu().numpy()[0]
    scenes = [clip_transformed(scene, i) for i in range(k)]
    got, st = _views(r, scenes, opaque, transparent, init, ids=True)
    draws = 0
    for i, sc in enumerate(scenes):
        want, wst = _single(r, sc, opaque, transparent, init, ids=True)
        _assert_layer(got, i, want, f"atrium K={k} fmt={fmt}")
        draws += wst.drawcall_count
    assert st.drawcall_count == draws
    r.close()


# ---------------------------------------------------------------- no bleed between layers
def test_no_bleed_into_the_next_layer(hip):
    w, h = 64, 40  # two tile rows per layer, the second partial
    rig = SC.Rig(hip, w, h)
    r = rig.r
    mesh = r.upload_mesh(SC.QUAD_IDX, SC.clip_quad(-1, -1, 1, 1, 0.5))
    obj = SC.objs([SC.render_object(mesh, rig.material(), 0, 6)])
    s0 = SC.identity_scene()
    s1 = SC.identity_scene()
    for i in range(16):  # view 1 has every vertex behind the camera (w = -1): nothing reaches its layer
        s1.viewproj[i] = 0.0
    s1.viewproj[0], s1.viewproj[5], s1.viewproj[10], s1.viewproj[15] = 1.0, 1.0, 1.0, -1.0
    init = np.full((h, w, 4), 0x1234, np.uint16)
    got, st = _views(r, [s0, s1], obj, None, init, ids=True)
    assert np.all(got["depth"][0] != 0.0), "view 0 covers its layer"
    assert np.all(got["depth"][1] == 0.0), "layer 1: depth cleared, nothing drawn"
    assert np.all(got["color"][1] == 0x1234), "layer 1 keeps its loaded colour in every row"
    assert np.all(got["ids"][1] == 0)
    r.close()


# ---------------------------------------------------------------- one result on every path
def test_same_layers_on_every_path(hip):
    """the host path (svr_draw_geometry_views; svr_draw_list_views with SVR_OPT_DEVICE_FLATTEN = 2) and the device path
    (svr_draw_list_views: list_views_kernel), with every tile-kernel variant"""
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    init = _layers(r, 1)[0].cpu().numpy()[0]
    scenes = [clip_transformed(scene, i) for i in range(6)]
    first, fst = _views(r, scenes, opaque, transparent, init, ids=True)
    runs = []
    for opt in ((A.OPT_COUNT_FRAGMENTS, 1), (A.OPT_TUNING, TUNE_NO_HIZ), (A.OPT_TUNING, TUNE_HIZ), (A.OPT_TUNING, 1),
                (A.OPT_TUNING, 8)):
        r.set_option(*opt)
        runs.append((f"geometry {opt}", _views(r, scenes, opaque, transparent, init, ids=True)))
        r.set_option(A.OPT_TUNING, 0)
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
    lst = r.create_draw_list(opaque, transparent)
    for opt in ((A.OPT_DEVICE_FLATTEN, 0), (A.OPT_DEVICE_FLATTEN, 2), (A.OPT_TUNING, TUNE_HIZ)):
        r.set_option(*opt)
        runs.append((f"list {opt}", _views(r, scenes, None, None, init, ids=True, lst=lst)))
        r.set_option(A.OPT_TUNING, 0)
        r.set_option(A.OPT_DEVICE_FLATTEN, 0)
    lst.close()
    for what, (got, st) in runs:
        for k in range(6):
            _assert_layer(got, k, {key: first[key][k] for key in first}, what)
        for f in ("triangle_count", "drawcall_count", "culled_draws"):
            assert getattr(st, f) == getattr(fst, f), f"{what}: {f}"


def test_debug_hooks_cover_every_layer(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    init = _layers(r, 1)[0].cpu().numpy()[0]
    scenes = [clip_transformed(scene, i) for i in range(3)]
    r.set_option(A.OPT_TILE_CYCLES, 1)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    per_layer = []
    for sc in scenes:
        _single(r, sc, opaque, transparent, init)
        per_layer.append(r.read_bins())
    rows = r.row_costs()
    _views(r, scenes, opaque, transparent, init)
    op, tr = r.read_bins()
    tpl = len(per_layer[0][0])
    assert len(op) == 3 * tpl
    np.testing.assert_array_equal(op, np.concatenate([b[0] for b in per_layer]))
    np.testing.assert_array_equal(tr, np.concatenate([b[1] for b in per_layer]))
    cyc = r.read_tile_cycles()
    assert cyc.shape == (3 * tpl, 4) and np.all(cyc.sum(axis=1) > 0)
    after = r.row_costs()  # still the last single-view pass
    np.testing.assert_array_equal(after[0], rows[0])
    assert after[1:] == rows[1:]
    r.close()


def test_replay_after_overflow(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    init = _layers(r, 1)[0].cpu().numpy()[0]
    scenes = [clip_transformed(scene, i) for i in range(6)]
    want, _ = _views(r, scenes, opaque, transparent, init, ids=True)
    before = r.get_stats().replayed_passes
    r.set_option(A.OPT_QUEUE_CAPS, 64)
    got, st = _views(r, scenes, opaque, transparent, init, ids=True)
    assert st.replayed_passes > before
    for k in range(6):
        _assert_layer(got, k, {key: want[key][k] for key in want}, "replayed")
    r.close()


# ---------------------------------------------------------------- the context's own targets
def test_context_targets_untouched_and_clear_lands(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    r.enable_ids()
    r.draw_geometry(scene, opaque, transparent)
    r.sync()
    ids_before, depth_before = r.read_ids(), r.read_depth()
    r.clear_color((0.25, 0.5, 0.75, 1.0))  # deferred: must land on the context's target, not in the layers
    init = _layers(r, 1)[0].cpu().numpy()[0]
    scenes = [clip_transformed(scene, i) for i in range(3)]
    got, _ = _views(r, scenes, opaque, transparent, init)
    col = r.read_color().view(np.uint16).reshape(h, w, 4)
    want = np.array([0x3400, 0x3800, 0x3a00, 0x3c00], np.uint16)
    assert np.all(col == want), "the deferred clear landed on the context's target"
    np.testing.assert_array_equal(r.read_depth(), depth_before)
    np.testing.assert_array_equal(r.read_ids(), ids_before)
    # clear_rgba = svr_clear_color + the single pass
    rgba = (0.1, 0.2, 0.3, 0.4)
    got, _ = _views(r, scenes, opaque, transparent, init, clear=rgba)
    r.clear_color(rgba)
    cleared = _init_color(r)
    for k, sc in enumerate(scenes):
        one, _ = _single(r, sc, opaque, transparent, cleared)
        _assert_layer(got, k, one, "clear_rgba")
    r.close()


# ---------------------------------------------------------------- refusals
def test_refusals(hip):
    w, h = 64, 40
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    color, depth, _ = _layers(r, 16)
    cp, dp = color.data_ptr(), depth.data_ptr()

    def code(scenes, c=cp, d=dp):
        with pytest.raises(pkg.SvrError) as e:
            r.draw_views(scenes, c, d, opaque, transparent)
        return e.value.code

    assert code([]) == -1
    assert code([scene] * 17) == -1
    assert code([scene], c=None) == -1
    assert code([scene], d=None) == -1
    odd = clip_transformed(scene, 1)
    odd.ambient_color[0] = 0.5
    assert code([scene, odd]) == -1
    r.set_scissor(0, 0, w, h - 1)
    assert code([scene]) == -5
    r.set_scissor(0, 0, w, h)
    r.set_row_interleave(2, 0)
    assert code([scene]) == -5
    r.set_row_interleave(1, 0)
    r.draw_views([scene] * 16, cp, dp, opaque, transparent)  # 16 layers of 2 tile rows: fine
    r.close()
    tall = hip.create(32, 1056)  # 33 tile rows: 16 views would be 528
    with pytest.raises(pkg.SvrError) as e:
        tall.draw_views([scene] * 16, cp, dp, None)
    assert e.value.code == -1
    tall.close()
