"""The camera motion blur pass (include/svr_motion.h) on the MI355X.

The reference is tests/native/motion_ref.cpp (motion_ref.py), the scalar restatement of DESIGN C67-C72 that
test_motion_ref.py pins on the CPU.  It is fed the colour and depth targets the HIP library itself holds before the pass, so
every comparison here is on bit patterns, over the whole target, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import lighting_ref as LR
import motion_ref as MR
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
# this frame's camera (position, yaw) against the previous one at the origin: a turn and a strafe
MOVES = {"yaw": ((0.0, 0.0, 0.0), 0.45), "strafe": ((3.0, 0.6, 0.0), 0.0)}


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


class Bound:
    """a context whose colour and depth targets are caller tensors holding `color` (uint16 [h, w, 4]) and `depth`"""

    def __init__(self, hip, color, depth):
        import torch
        self.torch = torch
        h, w = color.shape[:2]
        self.shape = (h, w)
        self.color = torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()).cuda()
        self.depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=f32).copy()).cuda()
        torch.cuda.synchronize()
        self.r = hip.create(w, h)
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())

    def put(self, color):
        h, w = self.shape
        self.r.sync()
        self.color.copy_(self.torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()))
        self.torch.cuda.synchronize()

    def read(self):
        self.r.sync()
        h, w = self.shape
        return self.color.cpu().numpy().view(np.uint16).reshape(h, w, 4)

    def read_depth(self):
        self.r.sync()
        return self.depth.cpu().numpy()

    def close(self):
        self.r.close()


def scene(w, h, seed):
    """a target with NaN, inf, negative and subnormal halves over a depth with cleared pixels"""
    cam = MR.Camera(w, h)
    return MR.random_hdr(w, h, seed, specials=True), cam.depth_of(MR.rolling_dist(w, h, seed + 1))


def shutter_for(depth, reproject, w, h, px=11.0):
    """the shutter at which the longest streak is px long: at 11 px the slower parts of these frames stay under 8 px for whole
    cell neighbourhoods, so both tap counts occur (n is 32 above 8)"""
    v = MR.velocity64(depth, reproject, 2.0, 1e9, w, h)["v"]
    return float(f32(2.0 * px / max(np.max(np.hypot(v[..., 0], v[..., 1])), 1e-3)))


def san_of(color):
    want = color.copy()
    want[..., :3] = MR.san_bits(color[..., :3])
    return want


def plane_depth(w, h, edge):
    """depth 1 left of column `edge` (near: reversed Z), 0 right of it"""
    return np.where(np.arange(w)[None, :] < edge, 1.0, 0.0).astype(f32) * np.ones((h, 1), f32)


# ---------------------------------------------------------------- 1. extents
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (7, 9), (33, 17), (96, 80)], ids=lambda e: f"{e[0]}x{e[1]}")
def test_extents(hip, extent):
    pytest.importorskip("torch")
    w, h = extent
    color, depth = scene(w, h, seed=61)
    assert (depth.view(np.uint32) == 0).any() or w * h < 8
    b = Bound(hip, color, depth)
    for name, (pos, yaw) in MOVES.items():
        rp = MR.camera_reproject(w, h, pos, yaw)
        shutter = shutter_for(depth, rp, w, h)
        for max_blur in (1.0, 4.3, 16.0):
            b.put(color)
            b.r.motion_blur_pass(rp, shutter, max_blur)
            got = b.read()
            want = MR.run_ref(color, depth, rp, shutter, max_blur)
            assert_color(got, want["color"], f"{w}x{h}, max_blur {max_blur}, {name}")
            assert np.array_equal(got[..., 3], color[..., 3])
            if w * h > 5000 and max_blur == 16.0:  # (a smaller target lies within one cell neighbourhood)
                L2 = (want["G"] >> np.uint64(32)).astype(np.uint32).view(f32)
                assert (L2 > 64).any() and ((L2 >= 0.25) & (L2 <= 64)).any(), "both tap counts"
    assert np.array_equal(b.read_depth().view(np.uint32), depth.view(np.uint32))
    b.close()


def test_odd_scissor(hip):
    pytest.importorskip("torch")
    w, h, scissor = 37, 23, (3, 5, 29, 15)
    color, depth = scene(w, h, seed=67)
    x0, y0, sw, sh = scissor
    guarded = np.full_like(color, GUARD)
    guarded[y0:y0 + sh, x0:x0 + sw] = color[y0:y0 + sh, x0:x0 + sw]
    b = Bound(hip, guarded, depth)
    b.r.set_scissor(*scissor)
    rp = MR.camera_reproject(w, h, *MOVES["strafe"])
    for max_blur in (4.3, 16.0):
        b.put(guarded)
        b.r.motion_blur_pass(rp, 1.0, max_blur)
        got = b.read()
        want = MR.run_ref(guarded, depth, rp, 1.0, max_blur, scissor=scissor)["color"]
        assert_color(got, want, f"odd scissor, max_blur {max_blur}")
        outside = np.ones((h, w), bool)
        outside[y0:y0 + sh, x0:x0 + sw] = False
        assert (got[outside] == GUARD).all(), "pixels outside the scissor keep their guard values"
        assert not (got[~outside][:, :3] == GUARD).any(), "and no tap read one: cells and clamps count from the scissor's origin"
        assert (got[~outside][:, :3] != guarded[~outside][:, :3]).any()
    b.close()


# ---------------------------------------------------------------- 2. invariants, library against library
def test_identity_and_a_closed_shutter(hip):
    pytest.importorskip("torch")
    w, h = 33, 17
    color, depth = scene(w, h, seed=71)
    assert (color == 0x7e00).any() and (color == 0xfc00).any()
    b = Bound(hip, color, depth)
    b.r.motion_blur_pass(GL.identity(), 1.0, 16.0)
    assert_color(b.read(), san_of(color), "identity: san(input)")
    rp = MR.camera_reproject(w, h, *MOVES["strafe"])
    for shutter, max_blur in ((0.0, 16.0), (1.0, 0.0)):
        b.put(color)
        b.r.motion_blur_pass(rp, shutter, max_blur)
        assert_color(b.read(), color, f"shutter {shutter}, max_blur {max_blur}: every bit stays, NaN halves included")
    b.close()


def test_a_static_front_plane_keeps_its_bits_and_a_moving_one_bleeds(hip):
    pytest.importorskip("torch")
    w, h, edge = 64, 32, 24
    color = MR.random_hdr(w, h, 73, specials=True)
    b = Bound(hip, color, plane_depth(w, h, edge))
    want = san_of(color)
    b.r.motion_blur_pass(MR.affine_reproject(ax=0.5, bx=-0.5), 1.0, 16.0)  # the plane still, the wall 8 px either way
    got = b.read().copy()
    assert np.array_equal(got[:, :edge], want[:, :edge]), "the still plane keeps its bits"
    assert (got[:, edge:, :3] != want[:, edge:, :3]).any(-1).mean() > 0.9, "the wall streaks"
    b.put(color)
    b.r.motion_blur_pass(MR.affine_reproject(ax=0.5), 1.0, 16.0)  # the plane 8 px either way, the wall still
    got = b.read()
    assert np.array_equal(got[:, edge + 9:], want[:, edge + 9:]), "wall pixels beyond the reach keep their bits"
    assert (got[:, edge:edge + 2, :3] != want[:, edge:edge + 2, :3]).any(-1).mean() > 0.9, "pixels next to the edge change"
    b.close()


def test_a_cells_tile_does_not_matter(hip):
    """the same image once under a scissor that starts 8 pixels (a cell) into the target and once over the whole target,
    whose first 8 columns repeat the image's first, which is what the clamp reads: every cell then lies in another place
    of its workgroup's tile, or in the next tile.  The reprojection is affine, so a velocity depends on its depth alone;
    max_blur 8: no tap and no cell neighbourhood (Rc = 1) reaches past the margin."""
    pytest.importorskip("torch")
    w, h, shift = 72, 32, 8
    color, depth = scene(w, h, seed=79)
    wide_c = np.concatenate([np.repeat(color[:, :1], shift, axis=1), color], axis=1)
    wide_d = np.concatenate([np.repeat(depth[:, :1], shift, axis=1), depth], axis=1)
    rp = MR.affine_reproject(ax=8.0, ay=-4.0)
    out = []
    for scissor in ((shift, 0, w, h), None):
        b = Bound(hip, wide_c, wide_d)
        if scissor:
            b.r.set_scissor(*scissor)
        b.r.motion_blur_pass(rp, 1.0, 8.0)
        out.append(b.read().copy())
        b.close()
    assert (out[0][:, shift:, :3] != wide_c[:, shift:, :3]).any(-1).mean() > 0.5
    assert_color(out[1][:, shift:], out[0][:, shift:], "shifted by a cell")


def sponza_reproject(sc):
    """the previous frame's camera: this frame's turned a little about the view's y axis"""
    proj, view = np.array(sc.proj, f32).reshape(4, 4), np.array(sc.view, f32).reshape(4, 4)
    prev = GL.matmul(proj, GL.matmul(GL.rotate(GL.identity(), f32(0.06), (0.0, 1.0, 0.0)), view))
    return GL.temporal_reproject(prev, GL.matmul(proj, view))


def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(sc, opaque, transparent)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    rp = sponza_reproject(sc)
    r.set_scissor(*scissor)
    r.motion_blur_pass(rp, 1.0, 12.0)
    got = r.read_color()
    assert_color(got, MR.run_ref(first["color"], first["depth"], rp, 1.0, 12.0, scissor=scissor)["color"], "motion blur under a scissor")
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
SHUTTER, MAX_BLUR = 1.0, 12.0  # on the sponza frame


def test_replayed_behind_an_overflowing_pass(hip):
    """the overflow is in the pass before the motion blur pass: it is void the first time and runs once in the replay"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, _ = T.setup_sponza(hip, w, h)
        rp = sponza_reproject(sc)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        r.motion_blur_pass(rp, SHUTTER, MAX_BLUR)  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            depth = r.read_depth()
            r.clear_color(CLEAR)
            r.draw_geometry(sc, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    once = MR.run_ref(forward, depth, rp, SHUTTER, MAX_BLUR)["color"]
    assert not np.array_equal(once, MR.run_ref(once, depth, rp, SHUTTER, MAX_BLUR)["color"]), "a second application would show"
    assert_color(frames[None][0], once, "forward frame, blurred once")
    assert_color(frames[64][0], frames[None][0], "motion blur pass behind a replayed pass")


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, motion blur pass, then a pass that overflows: the blur landed before the failing pass and the replay
    starts at that pass, so it is applied exactly once.  The last pass draws a third of the opaque objects and the
    transparent ones over the loaded depth, so most pixels still show what the motion blur pass left."""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
        rp = sponza_reproject(sc)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        blurred = MR.run_ref(r.read_color(), r.read_depth(), rp, SHUTTER, MAX_BLUR)["color"]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.motion_blur_pass(rp, SHUTTER, MAX_BLUR)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(sc, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    kept = np.all(frames[None][0] == blurred, axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the motion blur pass, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "motion blur pass in front of a replayed pass")


def test_a_deferred_clear_lands_before_the_pass(hip):
    """a uniform colour blurs to itself, so the pattern holds a negative half: the pass leaves san of it, 0, and a clear
    that landed behind the pass would leave the negative half itself"""
    w, h = 96, 64
    r = hip.create(w, h)
    pattern = (-1.0, 0.5, 12.0, 0.125)
    r.clear_color(pattern)  # deferred: no pass has taken it
    rp = MR.camera_reproject(w, h, *MOVES["yaw"])
    r.motion_blur_pass(rp, 1.0, 16.0)
    got = r.read_color()
    cleared = np.broadcast_to(LR.store(np.array(pattern, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    assert (cleared[..., 0] == 0xbc00).all()
    ref = MR.run_ref(cleared, r.read_depth(), rp, 1.0, 16.0)
    assert (MR.floats(ref["v"]) != 0).any(), "the cleared depth moves under a turn"
    want = ref["color"]
    assert (want[..., 0] == 0).all() and np.array_equal(want[..., 3], cleared[..., 3])
    assert_color(got, want, "clear, then motion blur pass")
    r.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color((3.0, 0.5, 12.0, 0.125))
    before = r.read_color()
    nan, inf = float("nan"), float("inf")
    rp = MR.camera_reproject(w, h, *MOVES["yaw"])
    good = dict(reproject=rp, shutter=1.0, max_blur=8.0)
    bad = [dict(shutter=v) for v in (-1.0, nan, inf)] + [dict(max_blur=v) for v in (-0.5, A.MOTION_MAX_BLUR + 0.5, nan, inf)]
    for v in (nan, inf, -inf):
        for at in ((0, 0), (2, 3), (3, 3)):
            m = rp.copy()
            m[at] = v
            bad.append(dict(reproject=m))
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.motion_blur_pass(**dict(good, **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_motion_blur_pass(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.motion_blur_pass(**good)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(r.read_color(), before, "refused calls change nothing")
    r.motion_blur_pass(**dict(good, shutter=4.0, max_blur=A.MOTION_MAX_BLUR))  # the largest there can be
    want = MR.run_ref(before, r.read_depth(), rp, 4.0, float(A.MOTION_MAX_BLUR))
    v = MR.floats(want["v"])
    assert np.hypot(v[..., 0], v[..., 1]).max() > 15.9  # the clamp at the largest max_blur is active
    assert_color(r.read_color(), want["color"], "the largest max_blur")
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color((0.3, 0.5, 0.2, 1.0))
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.motion_blur_pass(**good)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    r8.close()
