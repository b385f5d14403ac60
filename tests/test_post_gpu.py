"""The HDR post pass (include/svr_post.h) on the MI355X.

The reference is tests/native/post_ref.cpp (post_ref.py), the scalar restatement of DESIGN C22-C26 that test_post_ref.py
pins on the CPU.  It is fed the colour target the HIP library itself holds before the pass, so every comparison here is on
bit patterns, over the whole target, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import lighting_ref as LR
import post_ref as PR
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
PATTERN = (3.0, 0.5, 12.0, 0.125)
TUNE_NO_POLL = 16
GBUFFER = A.ATTR_NORMAL | A.ATTR_ALBEDO
OPS = {"clamp": A.TONEMAP_CLAMP, "reinhard": A.TONEMAP_REINHARD, "aces": A.TONEMAP_ACES}
POST = dict(exposure=0.8, bloom_threshold=1.0, bloom_intensity=0.3, bloom_levels=4, tonemap=A.TONEMAP_ACES)


def reference(color, scissor=None, **kw):
    p = dict(POST, **kw)
    return PR.run_ref(color, p["exposure"], p["bloom_threshold"], p["bloom_intensity"], p["bloom_levels"], p["tonemap"], scissor=scissor)


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


def point_lights(n, ref, seed):
    """n seeded point lights on the surfaces the lighting reference found, strong enough to push pixels well above 1"""
    rng = np.random.default_rng(seed)
    L = np.zeros(n, A.POINT_LIGHT_DTYPE)
    ok = ref["winner"] & np.all(np.isfinite(ref["position"]), axis=-1)
    ys, xs = np.nonzero(ok)
    pick = rng.integers(0, len(ys), n)
    L["position"] = ref["position"][ys[pick], xs[pick]] + rng.normal(0, 0.4, (n, 3)).astype(f32)
    L["radius"] = (10.0 ** rng.uniform(-0.3, 1.5, n)).astype(f32)
    L["color"] = rng.uniform(0.2, 1.0, (n, 3)).astype(f32)
    L["intensity"] = rng.uniform(5.0, 60.0, n).astype(f32)
    return L


class Bound:
    """a context whose colour and depth targets are caller tensors holding `color` (uint16 [h, w, 4]) and zeros"""

    def __init__(self, hip, color):
        import torch
        self.torch = torch
        h, w = color.shape[:2]
        self.shape = (h, w)
        self.color = torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()).cuda()
        self.depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.r = hip.create(w, h)
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())

    def read(self):
        self.r.sync()
        h, w = self.shape
        return self.color.cpu().numpy().view(np.uint16).reshape(h, w, 4)

    def close(self):
        self.r.close()


# ---------------------------------------------------------------- 1. the lit atrium
@pytest.fixture(scope="module")
def lit_atrium(hip):
    """the atrium's G-buffer at 160 x 96 and a relight() that puts the same HDR frame back into the colour target"""
    w, h = 160, 96
    r, scene, opaque, _ = T.setup_sponza(hip, w, h)
    r.enable_attributes(GBUFFER)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    args = (LR.inv_viewproj(scene.viewproj),) + LR.lighting_of(scene)
    unlit = LR.run_ref(r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO), *args)
    lights = point_lights(65, unlit, seed=31)

    def relight():
        r.light_pass(*args, lights=lights)
        return r.read_color()

    yield r, relight
    r.close()


@pytest.mark.parametrize("op", sorted(OPS))
def test_lit_atrium(lit_atrium, op):
    r, relight = lit_atrium
    before = relight()
    lit = PR.floats(before)[..., :3]
    assert (lit > 1.0).mean() > 0.02 and (lit < 1.0).mean() > 0.02, "the frame must hold values on both sides of 1"
    r.post_pass(**dict(POST, tonemap=OPS[op]))
    got = r.read_color()
    want = reference(before, tonemap=OPS[op])["color"]
    assert not np.array_equal(want, before)
    assert_color(got, want, f"lit atrium, {op}")
    assert PR.floats(got)[..., :3].max() <= 1.0


# ---------------------------------------------------------------- 2. random HDR planes in caller tensors
PLANE = (130, 67)  # w_0 = 65, h_0 = 34: the levels cross the 32- and 64-texel tile seams; with 8 levels the last are 1 x 1
ODD_SCISSOR = (3, 5, 117, 59)


@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("scissor", [None, ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_random_planes(hip, op, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    color = PR.random_hdr(w, h, seed=41)
    kw = dict(bloom_levels=8, tonemap=OPS[op])
    assert PR.level_extents(w, h, 8)[0] == (65, 34) and PR.level_extents(w, h, 8)[-1] == (1, 1)
    want = reference(color, scissor, **kw)["color"]
    b = Bound(hip, color)
    if scissor:
        b.r.set_scissor(*scissor)
    b.r.post_pass(**dict(POST, **kw))
    got = b.read()
    assert_color(got, want, f"random planes, {op}, scissor {scissor}")
    assert not b.depth.cpu().numpy().any()
    b.close()
    # nothing outside the scissor is read: NaN out there changes nothing inside
    if scissor:
        x0, y0, sw, sh = scissor
        poisoned = np.full_like(color, 0x7e00)
        poisoned[y0:y0 + sh, x0:x0 + sw] = color[y0:y0 + sh, x0:x0 + sw]
        b = Bound(hip, poisoned)
        b.r.set_scissor(*scissor)
        b.r.post_pass(**dict(POST, **kw))
        got2 = b.read()
        b.close()
        assert_color(got2[y0:y0 + sh, x0:x0 + sw], want[y0:y0 + sh, x0:x0 + sw], "inside, with NaN outside")
        outside = np.ones((h, w), bool)
        outside[y0:y0 + sh, x0:x0 + sw] = False
        assert (got2[outside] == 0x7e00).all()


@pytest.mark.parametrize("scissor", [(7, 9, 1, 1), (8, 3, 2, 1), (5, 4, 1, 5), (129, 66, 1, 1)], ids=["1x1", "2x1", "1x5", "last_pixel"])
def test_degenerate_scissors(hip, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    color = PR.random_hdr(w, h, seed=43, specials=False)
    b = Bound(hip, color)
    b.r.set_scissor(*scissor)
    for levels in (8, 1):
        before = b.read().copy()
        b.r.post_pass(**dict(POST, bloom_levels=levels, bloom_threshold=0.01))
        assert_color(b.read(), reference(before, scissor, bloom_levels=levels, bloom_threshold=0.01)["color"], f"scissor {scissor}, {levels} levels")
    b.close()


def test_bloom_off(hip):
    pytest.importorskip("torch")
    w, h = PLANE
    color = PR.random_hdr(w, h, seed=47)
    want = reference(color, bloom_levels=0)["color"]
    assert not np.array_equal(want, reference(color)["color"]), "the bloom must matter on this input"
    for kw in (dict(bloom_levels=0), dict(bloom_intensity=0.0)):
        b = Bound(hip, color)
        b.r.post_pass(**dict(POST, **kw))
        assert_color(b.read(), want, f"tone map alone ({kw})")
        b.close()


# ---------------------------------------------------------------- 3. closed forms (derived in test_post_ref.py)
@pytest.mark.parametrize("levels", [1, 8])
def test_constant_image(hip, levels):
    pytest.importorskip("torch")
    w, h, intensity = 37, 21, 0.01
    color = np.empty((h, w, 4), np.uint16)
    color[...] = PR.halves([3.0, 3.0, 3.0, 0.625])
    b = Bound(hip, color)
    b.r.post_pass(1.0, 1.0, intensity, levels, A.TONEMAP_REINHARD)
    got = b.read()
    b.close()
    hh = f32(np.float64(f32(intensity)) * (2.0 * levels) + 3.0)  # h = fma(intensity, 2 L, 3)
    assert (got[..., :3] == PR.h16(np.array([hh / (f32(1) + hh)], f32))[0]).all()
    assert (got[..., 3] == color[..., 3]).all()


def test_single_bright_texel(hip):
    pytest.importorskip("torch")
    color = np.zeros((48, 48, 4), np.uint16)
    color[21, 21, :3] = PR.halves(1024.0)
    b = Bound(hip, color)
    b.r.post_pass(1.0, 0.0, 1.0, 2, A.TONEMAP_REINHARD)
    got = b.read()
    b.close()
    assert np.array_equal(got, got.transpose(1, 0, 2)), "symmetric under swapping x and y"
    assert_color(got, PR.run_ref(color, 1.0, 0.0, 1.0, 2, PR.REINHARD)["color"], "single bright texel")


# ---------------------------------------------------------------- 4. nothing else moves
def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    r.set_scissor(*scissor)
    r.post_pass(**dict(POST, exposure=3.0))
    got = r.read_color()
    assert_color(got, reference(first["color"], scissor, exposure=3.0)["color"], "post under a scissor")
    x0, y0, sw, sh = scissor
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + sh, x0:x0 + sw] = True
    assert np.array_equal(got[~inside], first["color"][~inside]) and np.array_equal(got[..., 3], first["color"][..., 3])
    assert (got[inside][:, :3] != first["color"][inside][:, :3]).any()
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    assert np.array_equal(r.read_ids(), first["ids"])
    for a, plane in first["attr"].items():
        assert np.array_equal(r.read_attribute(a).view(np.uint32), plane.view(np.uint32)), a
    r.set_scissor(0, 0, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)  # a forward pass after it is what it was
    assert_color(r.read_color(), first["color"], "forward pass after a post pass")
    r.close()


# ---------------------------------------------------------------- 5. ordering
def test_replayed_behind_an_overflowing_pass(hip):
    """the overflow is in the pass before the post pass: the post pass is void the first time and runs once in the replay"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        r.post_pass(**dict(POST, exposure=3.0))  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    assert_color(frames[None][0], reference(forward, exposure=3.0)["color"], "forward frame, posted once")
    assert_color(frames[64][0], frames[None][0], "post pass behind a replayed pass")


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, post pass, then a pass that overflows: the post pass landed before the failing pass and the replay
    starts at that pass, so the post pass is applied exactly once.  The last pass draws a third of the opaque objects and
    the transparent ones over the loaded depth, so most pixels still show what the post pass left."""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        posted = reference(r.read_color(), exposure=3.0)["color"]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.post_pass(**dict(POST, exposure=3.0))
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    kept = np.all(frames[None][0] == posted, axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the post pass, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "post pass in front of a replayed pass")


def test_a_deferred_clear_lands_before_the_pass(hip):
    w, h = 96, 64
    r = hip.create(w, h)
    r.clear_color(PATTERN)  # deferred: no pass has taken it
    r.post_pass(**POST)
    got = r.read_color()
    cleared = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    assert_color(got, reference(cleared)["color"], "clear, then post pass")
    r.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color(PATTERN)
    before = r.read_color()
    nan, inf = float("nan"), float("inf")
    bad = [dict(exposure=v) for v in (0.0, -1.0, nan, inf)] + [dict(bloom_threshold=v) for v in (-1.0, nan, inf)] + \
          [dict(bloom_intensity=v) for v in (-0.5, nan, inf)] + [dict(bloom_levels=A.POST_MAX_LEVELS + 1), dict(tonemap=3)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.post_pass(**dict(POST, **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_post_pass(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.post_pass(**POST)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(r.read_color(), before, "refused calls change nothing")
    r.post_pass(**dict(POST, bloom_levels=A.POST_MAX_LEVELS))  # the most there can be
    assert_color(r.read_color(), reference(before, bloom_levels=A.POST_MAX_LEVELS)["color"], "the most levels")
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color(PATTERN)
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.post_pass(**POST)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    r8.close()


# ---------------------------------------------------------------- 7. present
def test_present_after_the_pass(hip):
    pytest.importorskip("torch")
    w, h = PLANE
    color = PR.random_hdr(w, h, seed=53, specials=False)
    b = Bound(hip, color)
    b.r.post_pass(**POST)
    got = b.r.read_swapchain(w, h)
    b.close()
    u = Bound(hip, reference(color)["color"])  # a target uploaded with the reference's output
    want = u.r.read_swapchain(w, h)
    u.close()
    assert np.array_equal(got, want)
    assert got[..., :3].max() == 255 and (got[..., :3] < 255).mean() > 0.3, "both clipped and unclipped pixels are presented"
