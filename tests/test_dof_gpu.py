"""The depth of field pass (include/svr_dof.h) on the MI355X.

The reference is tests/native/dof_ref.cpp (dof_ref.py), the scalar restatement of DESIGN C61-C66 that test_dof_ref.py pins
on the CPU.  It is fed the colour and depth targets the HIP library itself holds before the pass, so every comparison here
is on bit patterns, over the whole target, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import dof_ref as DR
import lighting_ref as LR
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
UNIT = DR.UnitCamera()
# (focus_distance, blur_scale) over rolling_dist's 1.8 .. 30 units and its cleared pixels: mostly in front of the focus,
# mostly behind it
FOCI = {"near_field": (25.0, 6.0), "far_field": (4.0, 20.0)}


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
    cam = DR.Camera(w, h)
    return cam, DR.random_hdr(w, h, seed, specials=True), cam.depth_of(DR.rolling_dist(w, h, seed + 1))


# ---------------------------------------------------------------- 1. extents
@pytest.mark.parametrize("extent", [(1, 1), (2, 3), (7, 9), (33, 17), (96, 80)], ids=lambda e: f"{e[0]}x{e[1]}")
def test_extents(hip, extent):
    pytest.importorskip("torch")
    w, h = extent
    cam, color, depth = scene(w, h, seed=61)
    assert (depth.view(np.uint32) == 0).any() or w * h < 8
    b = Bound(hip, color, depth)
    for max_radius in (1.0, 4.5, 16.0):
        for name, (focus, blur) in FOCI.items():
            b.put(color)
            b.r.dof_pass(*cam.terms, focus, blur, max_radius)
            got = b.read()
            want = DR.run_ref(color, depth, cam.terms, focus, blur, max_radius)
            assert_color(got, want["color"], f"{w}x{h}, max_radius {max_radius}, {name}")
            assert np.array_equal(got[..., 3], color[..., 3])
            if w * h > 64:
                c = DR.floats(want["prepared"][..., 3])
                assert ((c < 0).mean() > 0.5) == (name == "near_field") and np.abs(c).max() == max_radius
    assert np.array_equal(b.read_depth().view(np.uint32), depth.view(np.uint32))
    b.close()


def test_odd_scissor(hip):
    pytest.importorskip("torch")
    w, h, scissor = 37, 23, (3, 5, 29, 15)
    cam, color, depth = scene(w, h, seed=67)
    x0, y0, sw, sh = scissor
    guarded = np.full_like(color, GUARD)
    guarded[y0:y0 + sh, x0:x0 + sw] = color[y0:y0 + sh, x0:x0 + sw]
    b = Bound(hip, guarded, depth)
    b.r.set_scissor(*scissor)
    for max_radius in (4.5, 16.0):
        b.put(guarded)
        b.r.dof_pass(*cam.terms, 4.0, 9.25, max_radius)
        got = b.read()
        want = DR.run_ref(guarded, depth, cam.terms, 4.0, 9.25, max_radius, scissor=scissor)["color"]
        assert_color(got, want, f"odd scissor, max_radius {max_radius}")
        outside = np.ones((h, w), bool)
        outside[y0:y0 + sh, x0:x0 + sw] = False
        assert (got[outside] == GUARD).all(), "pixels outside the scissor keep their guard values"
        assert not (got[~outside][:, :3] == GUARD).any(), "and no tap read one: cells and clamps count from the scissor's origin"
        assert (got[~outside][:, :3] != guarded[~outside][:, :3]).any()
    b.close()


# ---------------------------------------------------------------- 2. invariants, library against library
def test_all_at_focus_and_zero_blur(hip):
    pytest.importorskip("torch")
    w, h = 33, 17
    color = DR.random_hdr(w, h, 71, specials=True)
    assert (color == 0x7e00).any() and (color == 0xfc00).any()
    depth = UNIT.depth_of(np.full((h, w), 4.0))
    b = Bound(hip, color, depth)
    b.r.dof_pass(*UNIT.terms, 4.0, 12.0, 16.0)
    want = color.copy()
    want[..., :3] = DR.san_bits(color[..., :3])
    assert_color(b.read(), want, "all at focus: san(input)")
    cam, _, rolling = scene(w, h, seed=71)
    b.close()
    b = Bound(hip, color, rolling)
    for blur, max_radius in ((0.0, 16.0), (6.0, 0.0)):
        b.r.dof_pass(*cam.terms, 4.0, blur, max_radius)
        assert_color(b.read(), color, f"blur_scale {blur}, max_radius {max_radius}: every bit stays, NaN halves included")
    b.close()


def test_foreground_bleeds_and_the_wall_beyond_reach_keeps_its_bits(hip):
    pytest.importorskip("torch")
    w, h, edge, max_radius = 64, 24, 8, 4.0
    reach = 4 + 8
    color = DR.random_hdr(w, h, 73, specials=True)
    b = Bound(hip, color, UNIT.depth_of(DR.plane_over_wall(w, h, edge, 1.0, 4.0)))
    b.r.dof_pass(*UNIT.terms, 4.0, 16.0, max_radius)
    got = b.read()
    assert np.array_equal(got[:, edge + reach:, :3], DR.san_bits(color[:, edge + reach:, :3])), "wall pixels beyond the reach keep their bits"
    assert (got[:, edge:edge + 2, :3] != DR.san_bits(color[:, edge:edge + 2, :3])).any(-1).mean() > 0.9, "pixels next to the edge change"
    b.close()


def test_a_cells_tile_does_not_matter(hip):
    """the same image once from the scissor's origin and once 8 pixels (a cell) to the right of it, behind a margin that
    repeats its first column, which is what the clamp reads: every cell then lies in another place of its workgroup's
    tile, or in the next tile.  max_radius 8: no tap and no cell neighbourhood (Rc = 1) reaches past the margin."""
    pytest.importorskip("torch")
    w, h, shift = 72, 32, 8
    cam, color, depth = scene(w, h, seed=79)
    wide_c = np.concatenate([np.repeat(color[:, :1], shift, axis=1), color], axis=1)
    wide_d = np.concatenate([np.repeat(depth[:, :1], shift, axis=1), depth], axis=1)
    out = []
    for c, d in ((color, depth), (wide_c, wide_d)):
        b = Bound(hip, c, d)
        b.r.dof_pass(*cam.terms, 4.0, 9.25, 8.0)
        out.append(b.read().copy())
        b.close()
    assert (out[0][..., :3] != color[..., :3]).any(-1).mean() > 0.5
    assert_color(out[1][:, shift:], out[0], "shifted by a cell")


def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(sc, opaque, transparent)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    terms = tuple(float(v) for v in GL.dof_depth_terms(np.array(sc.proj, f32).reshape(4, 4)))
    r.set_scissor(*scissor)
    r.dof_pass(*terms, 8.0, 10.0, 12.0)
    got = r.read_color()
    assert_color(got, DR.run_ref(first["color"], first["depth"], terms, 8.0, 10.0, 12.0, scissor=scissor)["color"], "depth of field under a scissor")
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
DOF = (8.0, 10.0, 12.0)  # focus_distance, blur_scale, max_radius on the sponza frame


def sponza_terms(sc):
    return tuple(float(v) for v in GL.dof_depth_terms(np.array(sc.proj, f32).reshape(4, 4)))


def test_replayed_behind_an_overflowing_pass(hip):
    """the overflow is in the pass before the depth of field pass: it is void the first time and runs once in the replay"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, _ = T.setup_sponza(hip, w, h)
        terms = sponza_terms(sc)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        r.dof_pass(*terms, *DOF)  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            depth = r.read_depth()
            r.clear_color(CLEAR)
            r.draw_geometry(sc, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    once = DR.run_ref(forward, depth, terms, *DOF)["color"]
    assert not np.array_equal(once, DR.run_ref(once, depth, terms, *DOF)["color"]), "a second application would show"
    assert_color(frames[None][0], once, "forward frame, blurred once")
    assert_color(frames[64][0], frames[None][0], "depth of field pass behind a replayed pass")


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, depth of field pass, then a pass that overflows: the blur landed before the failing pass and the replay
    starts at that pass, so it is applied exactly once.  The last pass draws a third of the opaque objects and the
    transparent ones over the loaded depth, so most pixels still show what the depth of field pass left."""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, sc, opaque, transparent = T.setup_sponza(hip, w, h)
        terms = sponza_terms(sc)
        r.clear_color(CLEAR)
        r.draw_geometry(sc, opaque, EMPTY)
        blurred = DR.run_ref(r.read_color(), r.read_depth(), terms, *DOF)["color"]
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.dof_pass(*terms, *DOF)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(sc, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    kept = np.all(frames[None][0] == blurred, axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the depth of field pass, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "depth of field pass in front of a replayed pass")


def test_a_deferred_clear_lands_before_the_pass(hip):
    """a uniform colour blurs to itself, so the pattern holds a negative half: the pass leaves san of it, 0, and a clear
    that landed behind the pass would leave the negative half itself"""
    w, h = 96, 64
    r = hip.create(w, h)
    pattern = (-1.0, 0.5, 12.0, 0.125)
    r.clear_color(pattern)  # deferred: no pass has taken it
    cam = DR.Camera(w, h)
    r.dof_pass(*cam.terms, 4.0, 9.25, 16.0)
    got = r.read_color()
    cleared = np.broadcast_to(LR.store(np.array(pattern, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    assert (cleared[..., 0] == 0xbc00).all()
    want = DR.run_ref(cleared, r.read_depth(), cam.terms, 4.0, 9.25, 16.0)["color"]
    assert (want[..., 0] == 0).all() and np.array_equal(want[..., 3], cleared[..., 3])
    assert_color(got, want, "clear, then depth of field pass")
    r.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color((3.0, 0.5, 12.0, 0.125))
    before = r.read_color()
    cam = DR.Camera(w, h)
    nan, inf = float("nan"), float("inf")
    good = dict(inv_z_scale=cam.terms[0], inv_z_bias=cam.terms[1], focus_distance=4.0, blur_scale=9.25, max_radius=8.0)
    bad = [dict(inv_z_scale=v) for v in (nan, inf, -inf)] + [dict(inv_z_bias=v) for v in (nan, inf)] + \
          [dict(focus_distance=v) for v in (0.0, -1.0, nan, inf)] + [dict(blur_scale=v) for v in (-1.0, nan, inf)] + \
          [dict(max_radius=v) for v in (-0.5, A.DOF_MAX_RADIUS + 0.5, nan, inf)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.dof_pass(**dict(good, **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_dof_pass(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.dof_pass(**good)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(r.read_color(), before, "refused calls change nothing")
    r.dof_pass(**dict(good, max_radius=A.DOF_MAX_RADIUS))  # the largest there can be
    want = DR.run_ref(before, r.read_depth(), cam.terms, 4.0, 9.25, float(A.DOF_MAX_RADIUS))
    assert DR.floats(want["prepared"][..., 3]).max() == 9.25  # the cleared depth: every pixel at the blur scale
    assert_color(r.read_color(), want["color"], "the largest radius")
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color((0.3, 0.5, 0.2, 1.0))
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.dof_pass(**good)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    r8.close()
