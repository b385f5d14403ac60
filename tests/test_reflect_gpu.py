"""The reflection pass (include/svr_reflect.h) on the MI355X.

The reference is tests/native/reflect_ref.cpp (reflect_ref.py), the scalar restatement of DESIGN C73-C79 that
test_reflect_ref.py pins on the CPU.  It is fed the colour, depth, normal and albedo planes the HIP library itself holds
before the pass, so every comparison here is on bit patterns, over the whole target, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import fog_ref as FR
import lighting_ref as LR
import reflect_ref as RR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
GL = pkg.glmath
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
TUNE_NO_POLL = 16
GUARD = 0x5a5a  # a finite half no result of these inputs is expected to produce by chance over a whole border
REFLECT = dict(max_distance=14.3, steps=16, refine=4, thickness=0.1, f0=0.3, intensity=0.9, distance_fade=0.5, edge_width=3.0, resolve=1,
               depth_tolerance=0.05, frame_index=3)
CORNERS = [dict(steps=1, refine=0, resolve=0), dict(steps=1, refine=8), dict(steps=64, refine=0), dict(steps=64, refine=8, resolve=0),
           dict(steps=64, refine=8), dict(thickness=0.0), dict(edge_width=0.0), dict(edge_width=1000.0), dict(resolve=0), dict()]


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


class Bound:
    """a context whose colour, depth, normal and albedo targets are caller tensors holding the G-buffer g (reflect_ref.cast's
    dict)"""

    def __init__(self, hip, g):
        import torch
        self.torch = torch
        h, w = g["depth"].shape
        self.shape = (h, w)
        self.color = torch.from_numpy(np.ascontiguousarray(g["color"]).view(np.int32).reshape(h, w, 2).copy()).cuda()
        self.planes = {k: torch.from_numpy(np.ascontiguousarray(g[k], dtype=f32).copy()).cuda() for k in ("depth", "normal", "albedo")}
        torch.cuda.synchronize()
        self.r = hip.create(w, h)
        self.r.bind_targets(self.color.data_ptr(), self.planes["depth"].data_ptr())
        self.r.bind_attribute_target(A.ATTR_NORMAL, self.planes["normal"].data_ptr())
        self.r.bind_attribute_target(A.ATTR_ALBEDO, self.planes["albedo"].data_ptr())

    def put(self, color):
        h, w = self.shape
        self.r.sync()
        self.color.copy_(self.torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()))
        self.torch.cuda.synchronize()

    def read(self):
        self.r.sync()
        h, w = self.shape
        return self.color.cpu().numpy().view(np.uint16).reshape(h, w, 4)

    def read_plane(self, k):
        self.r.sync()
        return self.planes[k].cpu().numpy()

    def close(self):
        self.r.close()


def scene(w, h, seed, **cast):
    """reflect_ref's floor, wall, box and sky at this extent, with NaN, inf, negative and subnormal halves sprinkled over the
    colour (at hit pixels and at source pixels alike) and stored normals of seeded lengths"""
    cam = RR.Camera(w, h, eye=(0.3, 2.6, 2.0), target=(0.0, 0.4, -4.0), fov_y=0.8)
    g = RR.cast(cam, wall_h=1.2, seed=seed, **cast)
    g["color"] = RR.random_hdr(w, h, seed + 1, specials=True)
    return cam, g


def planes_unchanged(b, g):
    for k in ("depth", "normal", "albedo"):
        assert np.array_equal(b.read_plane(k).view(np.uint32), np.ascontiguousarray(g[k], dtype=f32).view(np.uint32)), k


# ---------------------------------------------------------------- 1. extents and parameter corners
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (5, 4), (33, 17), (96, 80)], ids=lambda e: f"{e[0]}x{e[1]}")
def test_extents(hip, extent):
    pytest.importorskip("torch")
    w, h = extent
    cam, g = scene(w, h, seed=61)
    b = Bound(hip, g)
    hits = 0
    for corner in CORNERS:
        kw = dict(REFLECT, **corner)
        b.put(g["color"])
        b.r.reflect_pass(*cam.args(), **kw)
        got = b.read()
        want = RR.run_ref(g, *cam.args(), **kw)
        assert_color(got, want["color"], f"{w}x{h}, {corner}")
        assert np.array_equal(got[..., 3], g["color"][..., 3])
        hits += int((want["hit"][..., 0] >= 0).sum())
    assert hits > 0 or w * h < 64, "the corners must reflect something"
    planes_unchanged(b, g)
    b.close()


def test_odd_scissor(hip):
    pytest.importorskip("torch")
    w, h, scissor = 37, 23, (3, 5, 29, 15)
    cam, g = scene(w, h, seed=67)
    x0, y0, sw, sh = scissor
    guarded = np.full_like(g["color"], GUARD)
    guarded[y0:y0 + sh, x0:x0 + sw] = g["color"][y0:y0 + sh, x0:x0 + sw]
    g["color"] = guarded
    b = Bound(hip, g)
    b.r.set_scissor(*scissor)
    for corner in (dict(), dict(resolve=0), dict(edge_width=1000.0), dict(steps=64, refine=8)):
        kw = dict(REFLECT, **corner)
        b.put(guarded)
        b.r.reflect_pass(*cam.args(), **kw)
        got = b.read()
        want = RR.run_ref(g, *cam.args(), scissor=scissor, **kw)
        assert_color(got, want["color"], f"odd scissor, {corner}")
        outside = np.ones((h, w), bool)
        outside[y0:y0 + sh, x0:x0 + sw] = False
        assert (got[outside] == GUARD).all(), "pixels outside the scissor keep their guard values"
        assert (got[~outside][:, :3] != guarded[~outside][:, :3]).any()
        assert (want["hit"][..., 0] >= 0).sum() >= 10
    planes_unchanged(b, g)
    b.close()


def test_specials_at_hit_and_source_pixels(hip):
    """the colour's NaN, +-inf, negative halves and 65504 at pixels rays hit and at pixels that trace; depth, normal and
    albedo texels that are no numbers only ever enter arithmetic"""
    pytest.importorskip("torch")
    w, h = 33, 17
    cam, g = scene(w, h, seed=71)
    kw = dict(REFLECT, steps=64, refine=8)
    clean = RR.run_ref(g, *cam.args(), **kw)
    hit = clean["hit"][clean["hit"][..., 0] >= 0]
    assert len(hit) >= 30
    specials = [0x7e00, 0x7c00, 0xfc00, 0xc500, 0x7bff]
    for i, (hx, hy) in enumerate(hit[:10]):
        g["color"][hy, hx, i % 3] = specials[i % 5]
    ys, xs = np.nonzero(clean["hit"][..., 0] >= 0)
    for i in range(10):
        g["color"][ys[-1 - i], xs[-1 - i], i % 3] = specials[i % 5]
    g["depth"][1, 2:6] = (np.nan, np.inf, -1.0, 1e30)
    g["normal"][2, 3:6, 1] = (np.nan, np.inf, 1e30)
    g["albedo"][3, 4:6, 3] = (np.nan, 0.99999994)
    b = Bound(hip, g)
    for resolve in (0, 1):
        b.put(g["color"])
        b.r.reflect_pass(*cam.args(), **dict(kw, resolve=resolve))
        assert_color(b.read(), RR.run_ref(g, *cam.args(), **dict(kw, resolve=resolve))["color"], f"specials, resolve {resolve}")
    b.close()


def test_dither_follows_the_frame_index(hip):
    pytest.importorskip("torch")
    w, h = 33, 17
    cam, g = scene(w, h, seed=73)
    b = Bound(hip, g)
    frames = {}
    for name, kw in (("3", dict()), ("3 again", dict()), ("4", dict(frame_index=4)), ("3 + 2^32", dict(frame_index=3 + (1 << 32)))):
        kw = dict(REFLECT, refine=0, **kw)
        b.put(g["color"])
        b.r.reflect_pass(*cam.args(), **kw)
        frames[name] = b.read().copy()
        assert_color(frames[name], RR.run_ref(g, *cam.args(), **kw)["color"], f"frame index {name}")
    assert_color(frames["3 again"], frames["3"], "the same frame index, the same dither")
    assert_color(frames["3 + 2^32"], frames["3"], "the index is taken modulo 2^32")
    assert not np.array_equal(frames["4"], frames["3"]), "another frame index, another dither"
    b.close()
    # a frame of sky: no ray, and the frame index changes nothing
    sky = dict(g, depth=np.zeros((h, w), f32), albedo=np.zeros((h, w, 4), f32))
    b = Bound(hip, sky)
    for index in (3, 4):
        b.put(sky["color"])
        b.r.reflect_pass(*cam.args(), **dict(REFLECT, frame_index=index))
        frames[index] = b.read().copy()
        assert_color(frames[index], RR.run_ref(sky, *cam.args(), **dict(REFLECT, frame_index=index))["color"], f"sky, frame index {index}")
    assert_color(frames[4], frames[3], "nothing traces: the dither has nothing to move")
    b.close()


def test_a_ray_heading_behind_the_camera(hip):
    """a wall facing the camera and one long step: the first sample of most rays lies behind the camera (hw <= 0), which ends
    the march as a miss, as the fp64 statement finds"""
    pytest.importorskip("torch")
    w, h = 33, 17
    cam = RR.Camera(w, h, eye=(0.0, 1.0, 2.0), target=(0.0, 1.0, -6.0))
    g = RR.cast(cam, wall_h=8.0, box=None, seed=5)
    kw = dict(REFLECT, max_distance=12.0, steps=1, refine=0)
    m = RR.trace64(g, *cam.args(), **kw)
    assert m["behind_camera"].mean() > 0.3
    b = Bound(hip, g)
    b.r.reflect_pass(*cam.args(), **kw)
    want = RR.run_ref(g, *cam.args(), **kw)
    assert_color(b.read(), want["color"], "rays towards the camera")
    assert (want["hit"][m["behind_camera"]] == -1).all()
    b.close()


def test_intensity_zero_leaves_the_bits(hip):
    pytest.importorskip("torch")
    w, h = 33, 17
    cam, g = scene(w, h, seed=79)
    b = Bound(hip, g)
    b.r.reflect_pass(*cam.args(), **dict(REFLECT, intensity=0.0))
    assert_color(b.read(), g["color"], "intensity 0 leaves the target's bits")
    b.r.reflect_pass(*cam.args(), **REFLECT)
    assert not np.array_equal(b.read(), g["color"])
    b.close()


# ---------------------------------------------------------------- 2. nothing else moves
def sponza_args(sc):
    vp = np.array(sc.viewproj, f32).reshape(16)
    return (vp, LR.inv_viewproj(sc.viewproj), pkg.scenes.config3_camera()[0], *(float(v) for v in GL.dof_depth_terms(np.array(sc.proj, f32).reshape(4, 4))))


def gbuffer_of(r):
    return dict(color=r.read_color(), depth=r.read_depth(), normal=r.read_attribute(A.ATTR_NORMAL), albedo=r.read_attribute(A.ATTR_ALBEDO))


SPONZA = dict(REFLECT, max_distance=12.0, f0=0.5, intensity=1.0)


def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(sc, opaque, transparent)
    first = gbuffer_of(r)
    ids = r.read_ids()
    attr = {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}
    args = sponza_args(sc)
    r.set_scissor(*scissor)
    r.reflect_pass(*args, **SPONZA)
    got = r.read_color()
    want = RR.run_ref(first, *args, scissor=scissor, **SPONZA)
    assert (want["hit"][..., 0] >= 0).mean() > 0.02, "the frame must reflect something"
    assert_color(got, want["color"], "reflections under a scissor")
    x0, y0, sw, sh = scissor
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + sh, x0:x0 + sw] = True
    assert np.array_equal(got[~inside], first["color"][~inside]) and np.array_equal(got[..., 3], first["color"][..., 3])
    assert (got[inside][:, :3] != first["color"][inside][:, :3]).any()
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    assert np.array_equal(r.read_ids(), ids)
    for a, plane in attr.items():
        assert np.array_equal(r.read_attribute(a).view(np.uint32), plane.view(np.uint32)), a
    r.close()


# ---------------------------------------------------------------- 3. ordering
def test_replayed_behind_an_overflowing_pass(hip):
    """the overflow is in the pass before the reflection pass: it is void the first time and runs once in the replay"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, _ = T.setup_sponza(hip, w, h)
        r.enable_attributes(A.ATTR_ALL)
        args = sponza_args(sc)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        r.reflect_pass(*args, **SPONZA)  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            r.clear_color(CLEAR)
            r.draw_geometry(sc, opaque, EMPTY)
            forward = gbuffer_of(r)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    once = RR.run_ref(forward, *args, **SPONZA)["color"]
    assert not np.array_equal(once, RR.run_ref(dict(forward, color=once), *args, **SPONZA)["color"]), "a second application would show"
    assert_color(frames[None][0], once, "forward frame, reflected once")
    assert_color(frames[64][0], frames[None][0], "reflection pass behind a replayed pass")


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, reflection pass, then a pass that overflows: the reflection pass landed before the failing pass and the
    replay starts at that pass, so the reflections are applied exactly once.  The last pass draws a third of the opaque
    objects and the transparent ones over the loaded depth, so most pixels still show what the reflection pass left."""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
        r.enable_attributes(A.ATTR_ALL)
        args = sponza_args(sc)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        reflected = RR.run_ref(gbuffer_of(r), *args, **SPONZA)["color"]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.reflect_pass(*args, **SPONZA)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(sc, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    kept = np.all(frames[None][0] == reflected, axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the reflection pass, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "reflection pass in front of a replayed pass")


def test_a_deferred_clear_lands_before_the_pass(hip):
    pytest.importorskip("torch")
    w, h = 96, 64
    cam, g = scene(w, h, seed=83)
    b = Bound(hip, g)
    # (a uniform colour reflected in itself stays what it was; the negative green is what shows the order: the pass leaves
    # san of it, 0, and a clear landing behind the pass would leave the negative half)
    pattern = (3.0, -0.5, 12.0, 0.125)
    b.r.clear_color(pattern)  # deferred: no pass has taken it
    b.r.reflect_pass(*cam.args(), **REFLECT)
    got = b.read()
    cleared = np.broadcast_to(LR.store(np.array(pattern, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    assert_color(got, RR.run_ref(dict(g, color=cleared), *cam.args(), **REFLECT)["color"], "clear, then reflection pass")
    assert (cleared[..., 1] == 0xb800).all() and (got[..., 1] == 0).all()
    b.close()


# ---------------------------------------------------------------- 4. the chain
def test_light_reflect_fog_equals_the_three_restatements(hip):
    w, h = 96, 64
    r, sc, opaque, _ = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.clear_color(CLEAR)
    r.draw_geometry(sc, opaque, EMPTY)
    first = gbuffer_of(r)
    args = sponza_args(sc)
    inv, eye = args[1], args[2]
    lighting = LR.lighting_of(sc)
    fog = dict(density=0.06, height_falloff=0.15, height_base=1.0, max_distance=45.0, steps=7, fog_color=(0.5, 0.6, 0.7), sun_dir=(0.0, 1.0, 0.0, 0.0),
               sun_color=(0.0, 0.0, 0.0), edge_sharpness=2.0, frame_index=3)
    r.light_pass(inv, *lighting)
    r.reflect_pass(*args, **SPONZA)
    r.fog_pass(inv, eye, **fog)
    got = r.read_color()
    lit = LR.expected_color(first["color"], LR.run_ref(first["depth"], first["normal"], first["albedo"], inv, *lighting), A.COLOR_RGBA16F)
    reflected = RR.run_ref(dict(first, color=lit), *args, **SPONZA)
    assert (reflected["hit"][..., 0] >= 0).mean() > 0.02 and not np.array_equal(reflected["color"], lit)
    assert_color(got, FR.run_ref(reflected["color"], first["depth"], inv, eye, **fog)["color"], "light, reflect, fog")
    r.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals(hip):
    pytest.importorskip("torch")
    w, h = 64, 32
    cam, g = scene(w, h, seed=89)
    b = Bound(hip, g)
    r = b.r
    nan, inf = float("nan"), float("inf")
    bad = [dict(max_distance=v) for v in (0.0, -1.0, nan, inf)] + [dict(steps=v) for v in (0, A.REFLECT_MAX_STEPS + 1)] + \
          [dict(refine=A.REFLECT_MAX_REFINE + 1)] + [dict(thickness=v) for v in (-0.1, nan, inf)] + [dict(f0=v) for v in (-0.1, 1.5, nan)] + \
          [dict(intensity=v) for v in (-1.0, nan, inf)] + [dict(distance_fade=v) for v in (-0.1, 1.5, nan)] + \
          [dict(edge_width=v) for v in (-1.0, nan, inf)] + [dict(resolve=2)] + [dict(depth_tolerance=v) for v in (-0.1, nan, inf)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.reflect_pass(*cam.args(), **dict(REFLECT, **kw))
        assert e.value.code == -1, kw
    vp, inv, eye, zs, zb = cam.args()
    for args in ((np.where(np.arange(16) == 5, nan, vp), inv, eye, zs, zb), (vp, np.where(np.arange(16) == 9, inf, inv), eye, zs, zb),
                 (vp, inv, (0.0, nan, 0.0), zs, zb), (vp, inv, eye, nan, zb), (vp, inv, eye, zs, inf)):
        with pytest.raises(A.SvrError) as e:
            r.reflect_pass(*args, **REFLECT)
        assert e.value.code == -1
    assert hip.lib.svr_reflect_pass(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.reflect_pass(*cam.args(), **REFLECT)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(b.read(), g["color"], "refused calls change nothing")
    planes_unchanged(b, g)
    kw = dict(REFLECT, steps=A.REFLECT_MAX_STEPS, refine=A.REFLECT_MAX_REFINE)  # the most there can be
    r.reflect_pass(*cam.args(), **kw)
    assert_color(b.read(), RR.run_ref(g, *cam.args(), **kw)["color"], "the most steps and bisections")
    b.close()
    # a context without the planes
    bare = hip.create(w, h)
    bare.clear_color((3.0, 0.5, 12.0, 0.125))
    before = bare.read_color()
    with pytest.raises(A.SvrError, match="SVR_ATTR_NORMAL") as e:
        bare.reflect_pass(*cam.args(), **REFLECT)
    assert e.value.code == -1
    assert np.array_equal(bare.read_color(), before)
    bare.close()
    # a context-owned RGBA8 target
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.enable_attributes(A.ATTR_ALL)
    r8.clear_color((0.3, 0.5, 0.2, 1.0))
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.reflect_pass(*cam.args(), **REFLECT)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    r8.close()
