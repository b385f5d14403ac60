"""Depth-only passes (include/svr_depth.h) on the MI355X.

A depth-only pass over the opaque objects must leave the depth and ID targets bit for bit as the full pass over the same
opaque objects does, never touch colour, and report the full pass's stats with no shaded fragment: against the oracle's
full-size frames (tests/golden/full_frames.json) and against svr_draw_geometry of the HIP library itself on the edge-case
scenarios, draw lists, multiview layers, scissors, interleaved rows, deferred clears, replays and unfenced sequences."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T
from test_ids_gpu import TUNE_NO_SPLIT

_spec = importlib.util.spec_from_file_location("make_full_frames", os.path.join(T.GOLDEN_DIR, "make_full_frames.py"))
MF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MF)

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TUNE_NO_HIZ, TUNE_HIZ = 32, 64  # SVR_OPT_TUNING bits 5 and 6 (csrc/svr_device.h)
STATS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "binned_triangles", "bin_entries")


def _targets(r, n=1, ids=True, seed=5):
    """device targets of n layers: colour random bytes, depth and IDs garbage the pass must overwrite where it owns pixels"""
    h, w = r.height, r.width
    px = 8 if r.color_format == A.COLOR_RGBA16F else 4
    rng = np.random.default_rng(seed)
    color = torch.from_numpy(rng.integers(0, 256, (n, h, w, px), dtype=np.uint8)).cuda()
    depth = torch.from_numpy(rng.random((n, h, w), dtype=np.float32)).cuda()
    idt = torch.full((n, h, w, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if ids else None
    torch.cuda.synchronize()
    return color, depth, idt


def _host(t):
    return None if t is None else t.cpu().numpy()


def _pass(r, draw, ids=True, seed=5):
    """bind fresh targets, run draw(), fence; the targets before and after and the stats"""
    color, depth, idt = _targets(r, 1, ids, seed)
    before = {"color": _host(color)[0], "depth": _host(depth)[0]}
    if ids:
        before["ids"] = _host(idt)[0].view(np.uint32)
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    r.bind_id_target(idt.data_ptr() if ids else None)
    ret = draw()
    st = r.get_stats()
    torch.cuda.synchronize()
    out = {"color": _host(color)[0], "depth": _host(depth)[0]}
    if ids:
        out["ids"] = _host(idt)[0].view(np.uint32)
    r.bind_targets(None, None)
    r.bind_id_target(None)
    return before, out, st, ret


def _check_equivalent(r, scene, opaque, what, lst=None, ids=True):
    """depth-only pass (of opaque, or of the list lst whose opaque objects they are) == draw_geometry(opaque only) in
    depth, IDs and stats; colour untouched"""
    _, want, wst, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, None), ids)
    if lst is None:
        before, got, st, ret = _pass(r, lambda: r.draw_depth(scene, opaque), ids)
    else:
        before, got, st, ret = _pass(r, lambda: r.draw_list_depth(scene, lst), ids)
    T.assert_images_identical(got["depth"], want["depth"], f"{what} depth")
    if ids:
        T.assert_images_identical(got["ids"], want["ids"], f"{what} ids")
    assert np.array_equal(got["color"], before["color"]), f"{what}: the colour target was written"
    for f in STATS:
        assert getattr(st, f) == getattr(wst, f), f"{what}: {f}"
    assert st.shaded_fragments == 0, what
    return got, st


# ---------------------------------------------------------------- against the oracle's full-size frames
@pytest.mark.parametrize("flatten", [2, 1], ids=["host_flatten", "device_flatten"])
@pytest.mark.parametrize("name", list(MF.FRAMES))
def test_full_frames_hash_to_the_oracle_depth(hip, name, flatten):
    with open(MF.OUT) as f:
        doc = json.load(f)
    d = doc[name]
    w, h, instanced = MF.FRAMES[name]
    kw = dict(camera=S.config5_camera(), instances=S.config5_instances()) if instanced else {}
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=MF.TEX, **kw)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.set_option(A.OPT_DEVICE_FLATTEN, flatten)
    r.draw_depth(scene, opaque)
    depth = r.read_depth()
    st = r.get_stats()
    r.close()
    bad = [k for k in range(MF.STRIPS) if MF.sha(depth[slice(*MF.strip_rows(h, k))]) != d["depth_strips"][k]]
    assert not bad, f"{name}: depth differs from the oracle's in strips {bad}"
    assert MF.sha(depth) == d["depth"]
    assert int((depth > 0).sum()) == d["counters"]["covered_pixels"]
    assert st.shaded_fragments == 0


# ---------------------------------------------------------------- edge cases against draw_geometry(opaque only)
SCEN = sorted(SC.SCENARIOS)


def _capture(lib, name, mp):
    """the scenario's renderer, scene and objects just before its draw (the pass itself is not run)"""
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


@pytest.mark.parametrize("name", SCEN)
def test_scenarios_equal_the_opaque_pass(hip, name, monkeypatch):
    box = _capture(hip, name, monkeypatch)
    if "r" not in box:
        pytest.fail(f"{name}: no draw_geometry call")
    r, scene, opaque = box["r"], box["scene"], box["opaque"]
    for instr in (1, 0):
        r.set_option(A.OPT_COUNT_FRAGMENTS, instr)
        for tuning in (0, TUNE_NO_HIZ, TUNE_HIZ, TUNE_NO_SPLIT):
            r.set_option(A.OPT_TUNING, tuning)
            for flatten in (2, 1):
                r.set_option(A.OPT_DEVICE_FLATTEN, flatten)
                got, _ = _check_equivalent(r, scene, opaque, f"{name} instr={instr} tuning={tuning} flatten={flatten}")
                if tuning == 0 and flatten == 2:
                    split = got
                if tuning == TUNE_NO_SPLIT:  # the instances without the quarter path: also against the split pass itself
                    T.assert_images_identical(got["depth"], split["depth"], f"{name} instr={instr} no split: depth")
                    T.assert_images_identical(got["ids"], split["ids"], f"{name} instr={instr} no split: ids")
        r.set_option(A.OPT_DEVICE_FLATTEN, 2)  # (tuning: still TUNE_NO_SPLIT)
        got, _ = _check_equivalent(r, scene, opaque, f"{name} instr={instr} no split, without IDs", ids=False)
        T.assert_images_identical(got["depth"], split["depth"], f"{name} instr={instr} no split, without IDs: depth")
    r.set_option(A.OPT_TUNING, 0)
    r.set_option(A.OPT_DEVICE_FLATTEN, 0)
    _check_equivalent(r, scene, opaque, f"{name} without IDs", ids=False)
    r.close()


@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8])
def test_atrium_both_formats_and_debug_hooks(hip, fmt):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64, color_format=fmt)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    _check_equivalent(r, scene, opaque, f"atrium fmt={fmt}")
    r.draw_geometry(scene, opaque, transparent)
    r.sync()
    costs = r.row_costs()
    assert costs[0].size and costs[0].sum() > 0
    r.set_option(A.OPT_TILE_CYCLES, 1)
    r.trace_pixel(w // 2, h // 2)
    other = _clip_transformed(scene, 4)
    r.draw_depth(other, opaque)
    r.sync()
    after = r.row_costs()
    assert np.array_equal(after[0], costs[0]) and after[1:] == costs[1:], "row costs are the last colour pass's"
    assert not np.any(r.read_trace()), "a depth-only pass records no trace"
    cyc = r.read_tile_cycles()
    assert np.all(cyc[:, 1:] == 0) and np.any(cyc[:, 0] > 0), "a depth-only tile has phase A cycles only"
    op_bins, tr_bins = r.read_bins()
    assert op_bins.size == ((w + 31) // 32) * ((h + 31) // 32)
    assert np.all(tr_bins == 0) and np.any(op_bins > 0), "a depth-only pass bins no transparent triangle"
    r.close()


# ---------------------------------------------------------------- draw lists
def test_draw_lists(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    for flatten in (0, 2):
        r.set_option(A.OPT_DEVICE_FLATTEN, flatten)
        lst = r.create_draw_list(opaque, transparent)
        got_list, _ = _check_equivalent(r, scene, opaque, f"list flatten={flatten}", lst=lst)
        _, want, _, _ = _pass(r, lambda: r.draw_depth(scene, opaque))
        T.assert_images_identical(got_list["depth"], want["depth"], "list == draw_depth over its opaque objects")
        T.assert_images_identical(got_list["ids"], want["ids"], "list ids")
        _, full, _, _ = _pass(r, lambda: r.draw_list(scene, lst))  # transparent objects write neither depth nor IDs
        T.assert_images_identical(got_list["depth"], full["depth"], "list == draw_list depth")
        T.assert_images_identical(got_list["ids"], full["ids"], "list == draw_list ids")
        moved = opaque.copy()
        moved[0]["transform"][12] += 0.5
        moved[len(moved) // 2]["transform"][13] -= 0.25
        lst.update(0, moved)
        _, got, _, _ = _pass(r, lambda: r.draw_list_depth(scene, lst))
        _, want, _, _ = _pass(r, lambda: r.draw_depth(scene, moved))
        T.assert_images_identical(got["depth"], want["depth"], "after update")
        T.assert_images_identical(got["ids"], want["ids"], "ids after update")
        lst.close()
    r.set_option(A.OPT_DEVICE_FLATTEN, 0)
    lst = r.create_draw_list(opaque, transparent)
    r.destroy_mesh(int(opaque[0]["mesh"]))
    with pytest.raises(pkg.SvrError, match="no longer valid"):
        r.draw_list_depth(scene, lst)
    r.close()


# ---------------------------------------------------------------- multiview
def _lit(scene, k):
    out = _clip_transformed(scene, k)
    out.ambient_color[0] = 0.1 * k  # lighting may differ between the views of a depth-only pass
    out.sunlight_color[1] = 0.05 * k
    return out


def _clip_transformed(scene, k):
    """the scene seen through a per-view clip-space transform (as tests/test_views_gpu.py makes its views)"""
    a, s = 0.07 * k, 1.0 - 0.04 * k
    m = np.eye(4, dtype=np.float64)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = s * np.cos(a), -s * np.sin(a), s * np.sin(a), s * np.cos(a)
    m[0, 3], m[1, 3] = 0.06 * np.sin(1.7 * k), -0.05 * np.cos(1.3 * k)
    vp = np.array(scene.viewproj, dtype=np.float64).reshape(4, 4).T
    nvp = (m @ vp).astype(np.float32)
    out = A.SvrSceneData()
    ctypes.memmove(ctypes.addressof(out), ctypes.addressof(scene), ctypes.sizeof(out))
    for i, v in enumerate(nvp.T.reshape(16)):
        out.viewproj[i] = float(v)
    return out


@pytest.mark.parametrize("ids", [True, False], ids=["ids", "no_ids"])
@pytest.mark.parametrize("k", (1, 2, 6, 16))
def test_multiview_layers_equal_single_passes(hip, k, ids):
    w, h = 96, 54  # odd: every layer's last tile row is partial
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    scenes = [_lit(scene, i) for i in range(k)]
    singles, sums = [], {f: 0 for f in STATS}
    for sc in scenes:
        _, want, wst, _ = _pass(r, lambda: r.draw_depth(sc, opaque), ids)
        singles.append(want)
        for f in STATS:
            sums[f] += getattr(wst, f)
    lst = r.create_draw_list(opaque, transparent)
    # (form, tuning, instrumented; the last two: the instances without the quarter path, tile_depth_kernel<.., SPLIT = false, .., MV>)
    for form, tuning, instr in (("array", 0, 1), ("list", 0, 1), ("list", 0, 0), ("array", TUNE_NO_SPLIT, 1), ("array", TUNE_NO_SPLIT, 0)):
        r.set_option(A.OPT_TUNING, tuning)
        r.set_option(A.OPT_COUNT_FRAGMENTS, instr)
        _, depth, idt = _targets(r, k, ids)
        if form == "array":
            r.draw_depth_views(scenes, depth.data_ptr(), opaque, ids_ptr=idt.data_ptr() if ids else None)
        else:
            r.draw_list_depth_views(scenes, lst, depth.data_ptr(), ids_ptr=idt.data_ptr() if ids else None)
        st = r.get_stats()
        torch.cuda.synchronize()
        dh, ih = _host(depth), (_host(idt).view(np.uint32) if ids else None)
        for i, want in enumerate(singles):
            T.assert_images_identical(dh[i], want["depth"], f"{form} tuning={tuning} instr={instr} K={k} layer {i} depth")
            if ids:
                T.assert_images_identical(ih[i], want["ids"], f"{form} K={k} layer {i} ids")
        for f in (STATS if instr else ()):  # (an uninstrumented pass counts no fragments)
            assert getattr(st, f) == sums[f], f"{form} K={k}: {f}"
        assert st.shaded_fragments == 0
    lst.close()
    r.close()


def test_multiview_refusals(hip):
    w, h = 64, 40
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    color, depth, _ = _targets(r, 16, ids=False)
    lst = r.create_draw_list(opaque, transparent)
    args = A.SvrViewTargets()

    def code(call):
        with pytest.raises(pkg.SvrError) as e:
            call()
        return e.value.code

    arr = (A.SvrSceneData * 1)(scene)
    for c, clear in ((color.data_ptr(), None), (None, (ctypes.c_float * 4)(1, 1, 1, 1))):
        args.color, args.depth, args.ids = ctypes.c_void_p(c), ctypes.c_void_p(depth.data_ptr()), None
        args.clear_rgba = clear if clear is not None else ctypes.POINTER(ctypes.c_float)()
        op, n_op = r._objects(opaque)
        assert r.lib.lib.svr_draw_depth_views(r.h, 1, ctypes.addressof(arr), ctypes.byref(args), op, n_op, None) == -1
        assert b"NULL" in r.lib.lib.svr_last_error()
        assert r.lib.lib.svr_draw_list_depth_views(r.h, lst.handle, 1, ctypes.addressof(arr), ctypes.byref(args), None) == -1
    assert code(lambda: r.draw_depth_views([], depth.data_ptr(), opaque)) == -1
    assert code(lambda: r.draw_depth_views([scene] * 17, depth.data_ptr(), opaque)) == -1
    assert code(lambda: r.draw_depth_views([scene], None, opaque)) == -1
    r.set_scissor(0, 0, w, h - 1)
    assert code(lambda: r.draw_depth_views([scene], depth.data_ptr(), opaque)) == -5
    assert code(lambda: r.draw_list_depth_views([scene], lst, depth.data_ptr())) == -5
    r.set_scissor(0, 0, w, h)
    r.set_row_interleave(2, 0)
    assert code(lambda: r.draw_depth_views([scene], depth.data_ptr(), opaque)) == -5
    r.set_row_interleave(1, 0)
    r.draw_depth_views([scene] * 16, depth.data_ptr(), opaque)  # 16 layers of 2 tile rows: fine
    r.sync()
    lst.close()
    r.close()


# ---------------------------------------------------------------- scissor and interleave
def test_scissor_and_interleave_leave_other_rows(hip):
    w, h = 150, 170
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.set_scissor(13, 21, 101, 67)
    before, got, _, _ = _pass(r, lambda: r.draw_depth(scene, opaque))
    _check_equivalent(r, scene, opaque, "scissor")
    inside = np.zeros((h, w), bool)
    inside[21:88, 13:114] = True
    for key in ("depth", "ids"):
        assert np.array_equal(got[key][~inside], before[key][~inside]), f"scissor: {key} outside written"
    r.set_scissor(0, 0, w, h)
    for stride, off in ((2, 1), (3, 0)):
        r.set_row_interleave(stride, off)
        before, got, _, _ = _pass(r, lambda: r.draw_depth(scene, opaque))
        _check_equivalent(r, scene, opaque, f"interleave {stride},{off}")
        owned = np.zeros((h, w), bool)
        for t in range((h + 31) // 32):
            if t % stride == off:
                owned[t * 32:(t + 1) * 32] = True
        for key in ("depth", "ids"):
            assert np.array_equal(got[key][~owned], before[key][~owned]), f"interleave: {key} outside the owned rows written"
            assert not np.array_equal(got[key][owned], before[key][owned])
    r.set_row_interleave(1, 0)
    r.close()


# ---------------------------------------------------------------- the deferred clear
def test_deferred_clear_stays_with_colour(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    rgba = (0.25, 0.5, 0.75, 1.0)
    for flatten in (2, 1):
        r.set_option(A.OPT_DEVICE_FLATTEN, flatten)
        r.clear_color(rgba)
        r.draw_depth(scene, opaque)
        col = r.read_color().view(np.uint16).reshape(h, w, 4)
        assert np.all(col == np.array([0x3400, 0x3800, 0x3a00, 0x3c00], np.uint16)), "clear -> depth pass -> read_color"
        r.draw_geometry(scene, opaque, transparent)  # colour is now the frame: start the sequence from something else
        r.clear_color(rgba)
        r.draw_depth(scene, opaque)
        r.draw_geometry(scene, opaque, transparent)
        got = (r.read_color(), r.read_depth())
        r.clear_color(rgba)
        r.draw_geometry(scene, opaque, transparent)
        want = (r.read_color(), r.read_depth())
        T.assert_images_identical(got[0], want[0], "clear -> depth -> geometry colour")
        T.assert_images_identical(got[1], want[1], "clear -> depth -> geometry depth")
    r.close()


# ---------------------------------------------------------------- replay and pipelining
def test_replay_writes_the_targets_it_was_enqueued_with(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    _, roomy, _, _ = _pass(r, lambda: r.draw_depth(scene, opaque))
    before = r.get_stats().replayed_passes
    r.set_option(A.OPT_QUEUE_CAPS, 64)
    a = _targets(r, 1, True, seed=1)
    b = _targets(r, 1, True, seed=2)
    b_before = (_host(b[1]), _host(b[2]))
    r.bind_targets(a[0].data_ptr(), a[1].data_ptr())
    r.bind_id_target(a[2].data_ptr())
    r.draw_depth(scene, opaque)
    r.bind_targets(b[0].data_ptr(), b[1].data_ptr())  # before any fence: the replay must still write a
    r.bind_id_target(b[2].data_ptr())
    r.sync()
    st = r.get_stats()
    torch.cuda.synchronize()
    assert st.replayed_passes > before
    T.assert_images_identical(_host(a[1])[0], roomy["depth"], "replayed depth")
    T.assert_images_identical(_host(a[2])[0].view(np.uint32), roomy["ids"], "replayed ids")
    assert np.array_equal(_host(b[1]), b_before[0]) and np.array_equal(_host(b[2]), b_before[1]), "the later targets were written"
    r.bind_targets(None, None)
    r.bind_id_target(None)
    # a list pass replays from the version it was enqueued with
    lst = r.create_draw_list(opaque, transparent)
    r.bind_targets(a[0].data_ptr(), a[1].data_ptr())
    r.bind_id_target(a[2].data_ptr())
    r.draw_list_depth(scene, lst)
    moved = opaque.copy()
    moved[0]["transform"][12] += 3.0
    lst.update(0, moved)
    r.sync()
    torch.cuda.synchronize()
    T.assert_images_identical(_host(a[1])[0], roomy["depth"], "replayed list depth")
    r.bind_targets(None, None)
    r.bind_id_target(None)
    lst.close()
    r.close()


def test_unfenced_sequence_equals_fenced(hip):
    w, h = 96, 54
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    other = _clip_transformed(scene, 3)
    steps = [("colour", scene), ("depth", other), ("colour", other), ("depth", scene), ("colour", scene)]
    results = []
    for fenced in (True, False):
        tg = [_targets(r, 1, True, seed=10 + i) for i in range(len(steps))]
        for (kind, sc), (c, d, i) in zip(steps, tg):
            r.bind_targets(c.data_ptr(), d.data_ptr())
            r.bind_id_target(i.data_ptr())
            if kind == "colour":
                r.draw_geometry(sc, opaque, transparent)
            else:
                r.draw_depth(sc, opaque)
            if fenced:
                r.sync()
        r.sync()
        torch.cuda.synchronize()
        results.append([(_host(c), _host(d), _host(i)) for c, d, i in tg])
        r.bind_targets(None, None)
        r.bind_id_target(None)
    for k, (x, y) in enumerate(zip(*results)):
        for a, b, what in zip(x, y, ("colour", "depth", "ids")):
            assert np.array_equal(a, b), f"step {k} ({steps[k][0]}): {what}"
    r.close()
