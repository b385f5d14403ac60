"""The fog pass (include/svr_fog.h) on the MI355X.

The reference is tests/native/fog_ref.cpp (fog_ref.py), the scalar restatement of DESIGN C55-C60 that test_fog_ref.py pins
on the CPU.  It is fed the colour and depth targets the HIP library itself holds before the pass, so every comparison here
is on bit patterns, over the whole target, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import fog_ref as FR
import lighting_ref as LR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
TUNE_NO_POLL = 16
GUARD = 0x5a5a  # a finite half no fog result of these inputs is expected to produce by chance over a whole border
FOG = dict(density=0.06, height_falloff=0.15, height_base=1.0, max_distance=45.0, steps=7, fog_color=(0.5, 0.6, 0.7),
           sun_dir=(0.0, 1.0, 0.0, 0.0), sun_color=(6.0, 5.0, 4.0), anisotropy=0.4, shadow_bias=0.002, edge_sharpness=2.0, frame_index=3)


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


class Bound:
    """a context whose colour and depth targets are caller tensors holding `color` (uint16 [h, w, 4]) and `depth`; a shadow
    map, if given, lives in a third tensor"""

    def __init__(self, hip, color, depth, shadow=None):
        import torch
        self.torch = torch
        h, w = color.shape[:2]
        self.shape = (h, w)
        self.color = torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()).cuda()
        self.depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=f32).copy()).cuda()
        self.shadow = torch.from_numpy(np.ascontiguousarray(shadow, dtype=f32).copy()).cuda() if shadow is not None else None
        torch.cuda.synchronize()
        self.r = hip.create(w, h)
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())

    def put(self, color):
        h, w = self.shape
        self.r.sync()
        self.color.copy_(self.torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()))
        self.torch.cuda.synchronize()

    def shadow_args(self, M_light):
        hs, ws = self.shadow.shape
        return dict(shadow_ptr=self.shadow.data_ptr(), shadow_size=(ws, hs), shadow_viewproj=FR.colmajor(M_light))

    def read(self):
        self.r.sync()
        h, w = self.shape
        return self.color.cpu().numpy().view(np.uint16).reshape(h, w, 4)

    def read_depth(self):
        self.r.sync()
        return self.depth.cpu().numpy()

    def close(self):
        self.r.close()


M_LIGHT, SUN_DIR = FR.ortho_light()
SHADOW16 = FR.slab_map(16, M_LIGHT, seed=5)


def scene(w, h, seed):
    """a target with NaN, inf, negative and subnormal halves over a depth with cleared pixels"""
    cam = FR.Camera(w, h)
    return cam, FR.random_hdr(w, h, seed, specials=True), cam.depth_of(FR.rolling_depth(w, h, seed + 1))


def ref_kw(kw, shadowed):
    """the restatement's keywords of the library call's"""
    out = {k: v for k, v in kw.items() if not k.startswith("shadow_") or k == "shadow_bias"}
    if shadowed:
        out["shadow_viewproj"] = FR.colmajor(M_LIGHT)
    return out


# ---------------------------------------------------------------- 1. extents
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (5, 4), (33, 17), (96, 80)], ids=lambda e: f"{e[0]}x{e[1]}")
def test_extents(hip, extent):
    pytest.importorskip("torch")
    w, h = extent
    cam, color, depth = scene(w, h, seed=61)
    assert (depth.view(np.uint32) == 0).any() or w * h < 8
    b = Bound(hip, color, depth, SHADOW16)
    for steps in (1, 7, 64):
        for shadowed in (False, True):
            for falloff in (0.0, 0.15):
                kw = dict(FOG, steps=steps, height_falloff=falloff)
                b.put(color)
                b.r.fog_pass(cam.inv, cam.eye, **kw, **(b.shadow_args(M_LIGHT) if shadowed else {}))
                got = b.read()
                want = FR.run_ref(color, depth, cam.inv, cam.eye, shadow=SHADOW16 if shadowed else None, **ref_kw(kw, shadowed))["color"]
                assert_color(got, want, f"{w}x{h}, {steps} steps, map {shadowed}, falloff {falloff}")
                assert np.array_equal(got[..., 3], color[..., 3])
    assert np.array_equal(b.read_depth().view(np.uint32), depth.view(np.uint32))
    b.close()


def test_odd_scissor(hip):
    pytest.importorskip("torch")
    w, h, scissor = 37, 23, (3, 5, 29, 15)
    cam, color, depth = scene(w, h, seed=67)
    x0, y0, sw, sh = scissor
    guarded = np.full_like(color, GUARD)
    guarded[y0:y0 + sh, x0:x0 + sw] = color[y0:y0 + sh, x0:x0 + sw]
    b = Bound(hip, guarded, depth, SHADOW16)
    b.r.set_scissor(*scissor)
    for shadowed in (False, True):
        b.put(guarded)
        b.r.fog_pass(cam.inv, cam.eye, **FOG, **(b.shadow_args(M_LIGHT) if shadowed else {}))
        got = b.read()
        want = FR.run_ref(guarded, depth, cam.inv, cam.eye, scissor=scissor, shadow=SHADOW16 if shadowed else None, **ref_kw(FOG, shadowed))["color"]
        assert_color(got, want, f"odd scissor, map {shadowed}")
        outside = np.ones((h, w), bool)
        outside[y0:y0 + sh, x0:x0 + sw] = False
        assert (got[outside] == GUARD).all(), "pixels outside the scissor keep their guard values"
        assert (got[~outside][:, :3] != guarded[~outside][:, :3]).any()
    b.close()


def test_perspective_light(hip):
    """the case test_fog_ref.py's test_perspective_light_outside_or_behind_is_lit classifies: an eighth of the samples lie
    behind the light, where C18's `q.w > 0` decides, and half outside the map"""
    pytest.importorskip("torch")
    w, h = 33, 17
    cam, color, depth = scene(w, h, seed=61)
    M_spot, sun = FR.spot_light()
    smap = FR.spot_map(16, seed=5)
    kw = dict(FOG, sun_dir=sun)
    b = Bound(hip, color, depth, smap)
    b.r.fog_pass(cam.inv, cam.eye, **kw, **b.shadow_args(M_spot))
    got = b.read()
    want = FR.run_ref(color, depth, cam.inv, cam.eye, shadow=smap, shadow_viewproj=FR.colmajor(M_spot), **ref_kw(kw, False))["color"]
    assert_color(got, want, "a perspective light")
    assert not np.array_equal(want, FR.run_ref(color, depth, cam.inv, cam.eye, **ref_kw(kw, False))["color"]), "the map must matter"
    b.close()


# ---------------------------------------------------------------- 2. invariants, library against library
def test_invariants(hip):
    pytest.importorskip("torch")
    w, h = 33, 17
    cam, color, depth = scene(w, h, seed=71)
    lit_map, dark_map = np.zeros((16, 16), f32), np.full((16, 16), 4.0, f32)  # nothing above the ground; an occluder above everything
    # a light whose map covers every sample: at 45 units the frustum is 48 wide each way, and a sample outside the map is lit
    M_big, _ = FR.ortho_light(center=(0.0, 0.0, -20.0), half=64.0, height=200.0)
    results = {}
    for name, shadow, kw in (("no_map", None, {}), ("all_lit", lit_map, {}), ("all_dark", dark_map, {}), ("no_sun", None, dict(sun_color=(0.0, 0.0, 0.0))),
                             ("frame_4", None, dict(frame_index=4)), ("zero", None, dict(density=0.0))):
        b = Bound(hip, color, depth, shadow)
        b.r.fog_pass(cam.inv, cam.eye, **dict(FOG, **kw), **(b.shadow_args(M_big) if shadow is not None else {}))
        results[name] = b.read().copy()
        assert np.array_equal(b.read_depth().view(np.uint32), depth.view(np.uint32)), name
        assert np.array_equal(results[name][..., 3], color[..., 3]), name
        b.close()
    assert_color(results["all_lit"], results["no_map"], "an all-lit map equals no map")
    assert_color(results["all_dark"], results["no_sun"], "an all-occluding map equals no sun")
    assert not np.array_equal(results["no_sun"], results["no_map"]), "the sun must matter on this input"
    assert not np.array_equal(results["frame_4"], results["no_map"]), "two frame indices differ"
    assert_color(results["zero"], color, "density 0 leaves the target's bits")


def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(sc, opaque, transparent)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    inv, eye = LR.inv_viewproj(sc.viewproj), pkg.scenes.config3_camera()[0]
    r.set_scissor(*scissor)
    r.fog_pass(inv, eye, **FOG)
    got = r.read_color()
    assert_color(got, FR.run_ref(first["color"], first["depth"], inv, eye, scissor=scissor, **FOG)["color"], "fog under a scissor")
    x0, y0, sw, sh = scissor
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + sh, x0:x0 + sw] = True
    assert np.array_equal(got[~inside], first["color"][~inside]) and np.array_equal(got[..., 3], first["color"][..., 3])
    assert (got[inside][:, :3] != first["color"][inside][:, :3]).any()
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    assert np.array_equal(r.read_ids(), first["ids"])
    for a, plane in first["attr"].items():
        assert np.array_equal(r.read_attribute(a).view(np.uint32), plane.view(np.uint32)), a
    r.close()


# ---------------------------------------------------------------- 3. ordering
def test_replayed_behind_an_overflowing_pass(hip):
    """the overflow is in the pass before the fog pass: the fog pass is void the first time and runs once in the replay"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, _ = T.setup_sponza(hip, w, h)
        inv, eye = LR.inv_viewproj(sc.viewproj), pkg.scenes.config3_camera()[0]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        r.fog_pass(inv, eye, **FOG)  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            depth = r.read_depth()
            r.clear_color(CLEAR)
            r.draw_geometry(sc, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    once = FR.run_ref(forward, depth, inv, eye, **FOG)["color"]
    assert not np.array_equal(once, FR.run_ref(once, depth, inv, eye, **FOG)["color"]), "a second application would show"
    assert_color(frames[None][0], once, "forward frame, fogged once")
    assert_color(frames[64][0], frames[None][0], "fog pass behind a replayed pass")


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, fog pass, then a pass that overflows: the fog pass landed before the failing pass and the replay starts
    at that pass, so the fog is applied exactly once.  The last pass draws a third of the opaque objects and the transparent
    ones over the loaded depth, so most pixels still show what the fog pass left."""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
        inv, eye = LR.inv_viewproj(sc.viewproj), pkg.scenes.config3_camera()[0]
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        fogged = FR.run_ref(r.read_color(), r.read_depth(), inv, eye, **FOG)["color"]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.fog_pass(inv, eye, **FOG)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(sc, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    kept = np.all(frames[None][0] == fogged, axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the fog pass, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "fog pass in front of a replayed pass")


def test_a_deferred_clear_lands_before_the_pass(hip):
    w, h = 96, 64
    r = hip.create(w, h)
    pattern = (3.0, 0.5, 12.0, 0.125)
    r.clear_color(pattern)  # deferred: no pass has taken it
    cam = FR.Camera(w, h)
    r.fog_pass(cam.inv, cam.eye, **FOG)
    got = r.read_color()
    cleared = np.broadcast_to(LR.store(np.array(pattern, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    assert_color(got, FR.run_ref(cleared, r.read_depth(), cam.inv, cam.eye, **FOG)["color"], "clear, then fog pass")
    r.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals(hip):
    pytest.importorskip("torch")
    import torch
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color((3.0, 0.5, 12.0, 0.125))
    before = r.read_color()
    cam = FR.Camera(w, h)
    smap = torch.zeros((16, 16), dtype=torch.float32, device="cuda")
    nan, inf = float("nan"), float("inf")
    bad = [dict(density=v) for v in (-1.0, nan, inf)] + [dict(height_falloff=v) for v in (-0.5, nan, inf)] + \
          [dict(max_distance=v) for v in (0.0, -1.0, nan, inf)] + [dict(steps=v) for v in (0, A.FOG_MAX_STEPS + 1)] + \
          [dict(anisotropy=v) for v in (1.0, -1.0, 1.5, nan)] + [dict(edge_sharpness=v) for v in (-1.0, nan, inf)] + \
          [dict(shadow_ptr=smap.data_ptr(), shadow_size=s, shadow_viewproj=np.eye(4)) for s in ((0, 16), (16, 0), ((1 << 24) + 1, 16), (16, (1 << 24) + 1))]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.fog_pass(cam.inv, cam.eye, **dict(FOG, **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_fog_pass(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.fog_pass(cam.inv, cam.eye, **FOG)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(r.read_color(), before, "refused calls change nothing")
    r.fog_pass(cam.inv, cam.eye, **dict(FOG, steps=A.FOG_MAX_STEPS))  # the most there can be
    assert_color(r.read_color(), FR.run_ref(before, r.read_depth(), cam.inv, cam.eye, **dict(FOG, steps=A.FOG_MAX_STEPS))["color"], "the most steps")
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color((0.3, 0.5, 0.2, 1.0))
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.fog_pass(cam.inv, cam.eye, **FOG)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    r8.close()
