"""Temporal antialiasing (include/svr_temporal.h) on the MI355X.

The reference is tests/native/temporal_ref.cpp (temporal_ref.py), the scalar restatement of DESIGN C27-C31 that
test_temporal_ref.py pins on the CPU.  It is fed the colour, depth and history the HIP library itself holds before the
pass, so every comparison here is on bit patterns, over the whole target, with no tolerance; the one exception is the
convergence test, whose bound is derived there."""
import numpy as np
import pytest

import __graft_entry__ as g
import lighting_ref as LR
import native_ref as N
import post_ref as PR
import svr_testlib as T
import temporal_ref as TR

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
PATTERN = (3.0, 0.5, 12.0, 0.125)
TUNE_NO_POLL = 16
ID = TR.identity()
BLEND = 0.3


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


def inside_of(shape, scissor):
    m = np.zeros(shape, bool)
    x0, y0, sw, sh = scissor
    m[y0:y0 + sh, x0:x0 + sw] = True
    return m


def assert_history(r, want, scissor, what, valid=True):
    """the history the next resolve reads: the reference's inside the scissor (outside it nothing ever reads it)"""
    got, flag = r.read_temporal_history()
    m = inside_of(got.shape[:2], scissor)
    assert_color(np.where(m[..., None], got, 0), np.where(m[..., None], want, 0), what + ", history")
    assert flag == valid, what


def san_bits(color):
    """h16(san(I)) on the RGB halves, alpha as it is"""
    out = color.copy()
    out[..., :3] = N.san_bits(color[..., :3])
    return out


def viewproj(camera, w, h):
    pos, pitch, yaw = camera
    return GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[2]


def two_cameras(w, h):
    """a few degrees and a few centimetres apart: with depths in [0, 1] (0.1 units and more from the eye) part of the frame
    reprojects inside the image and part of it does not"""
    pos, pitch, yaw = (0.0, 2.0, 0.0), 0.1, 1.5
    return GL.temporal_reproject(viewproj((pos, pitch, yaw), w, h), viewproj(((-0.03, 2.02, 0.02), pitch, yaw + 0.05), w, h))


class Bound:
    """a context whose colour and depth targets are caller tensors"""

    def __init__(self, hip, color, depth):
        import torch
        self.torch = torch
        h, w = depth.shape
        self.shape = (h, w)
        self.color = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda")
        self.depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=f32)).cuda()
        self.r = hip.create(w, h)
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())
        self.upload(color)

    def upload(self, color):
        """the next frame's colour (after a fence: nothing of the context is in flight)"""
        self.r.sync()
        h, w = self.shape
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


# ---------------------------------------------------------------- 1. random planes in caller tensors
PLANE = (130, 67)  # 5 x 3 tiles of 32: both extents cross tile seams and end in a partial tile
ODD_SCISSOR = (3, 5, 117, 59)


def run_frames(hip, colors, depth, scissor, reproject, flags=0):
    """three consecutive resolves -> per frame (colour read back, reference); both ping-pong images are read and written"""
    w, h = PLANE
    full = scissor or (0, 0, w, h)
    b = Bound(hip, colors[0], depth)
    if scissor:
        b.r.set_scissor(*scissor)
    hist, out = np.zeros((h, w, 4), np.uint16), []
    for k, color in enumerate(colors):
        if k:
            b.upload(color)
        b.r.temporal_resolve(reproject, BLEND, flags)
        got = b.read().copy()
        want = TR.run_ref(color, depth, hist, reproject, BLEND, flags, history_valid=k > 0, scissor=scissor)
        assert_history(b.r, want["history"], full, f"frame {k}")
        hist = want["history"]
        out.append((got, want))
    assert np.array_equal(b.read_depth().view(np.uint32), np.ascontiguousarray(depth, f32).view(np.uint32))
    b.close()
    return out


@pytest.mark.parametrize("flags", [0, A.TEMPORAL_NO_CLAMP], ids=["clamp", "no_clamp"])
@pytest.mark.parametrize("scissor", [None, ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_random_planes(hip, scissor, flags):
    pytest.importorskip("torch")
    w, h = PLANE
    colors = [PR.random_hdr(w, h, seed=s) for s in (61, 62, 63)]
    depth = TR.random_depth(w, h, seed=64)
    m = two_cameras(w, h)
    full = scissor or (0, 0, w, h)
    frames = run_frames(hip, colors, depth, scissor, m, flags)
    for k, (got, want) in enumerate(frames):
        assert_color(got, want["color"], f"random planes, frame {k}, scissor {scissor}")
    used = frames[2][1]["valid"][inside_of((h, w), full)].mean()
    assert 0.1 <= used <= 0.9, f"{used:.3f} of the pixels of frame 2 use the history"
    assert not frames[0][1]["valid"].any()
    if scissor and not flags:
        # nothing outside the scissor is read: NaN out there, in colour and depth, changes nothing inside
        m_in = inside_of((h, w), scissor)
        poisoned = [np.where(m_in[..., None], c, np.uint16(0x7e00)) for c in colors]
        bad_depth = np.where(m_in, depth, f32(np.nan)).astype(f32)
        b = Bound(hip, poisoned[0], bad_depth)
        b.r.set_scissor(*scissor)
        for k, color in enumerate(poisoned):
            if k:
                b.upload(color)
            b.r.temporal_resolve(m, BLEND, flags)
            got = b.read()
            assert_color(np.where(m_in[..., None], got, 0), np.where(m_in[..., None], frames[k][1]["color"], 0), f"inside, NaN outside, frame {k}")
            assert (got[~m_in] == 0x7e00).all()
        b.close()


@pytest.mark.parametrize("scissor", [(7, 9, 1, 1), (8, 3, 2, 1), (5, 4, 1, 5), (129, 66, 1, 1)], ids=["1x1", "2x1", "1x5", "last_pixel"])
def test_degenerate_scissors(hip, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    colors = [PR.random_hdr(w, h, seed=s, specials=False) for s in (65, 66)]
    depth = np.full((h, w), 0.5, f32)
    b = Bound(hip, colors[0], depth)
    b.r.set_scissor(*scissor)
    hist = np.zeros((h, w, 4), np.uint16)
    for k, color in enumerate(colors):
        if k:
            b.upload(color)
        b.r.temporal_resolve(ID, BLEND)
        want = TR.run_ref(color, depth, hist, ID, BLEND, history_valid=k > 0, scissor=scissor)
        assert_color(b.read(), want["color"], f"scissor {scissor}, frame {k}")
        assert_history(b.r, want["history"], scissor, f"scissor {scissor}, frame {k}")
        assert want["valid"][inside_of((h, w), scissor)].all() == (k > 0)
        hist = want["history"]
    b.close()


# ---------------------------------------------------------------- 2. the atrium under a yaw step
def test_atrium_under_a_yaw_step(hip):
    w, h = 160, 96
    pos, pitch, yaw = S.config3_camera()
    cams = [(pos, pitch, yaw), (pos, pitch, yaw + 0.06)]
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, camera=cams[0])
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    first = r.read_color()
    r.temporal_resolve(ID, BLEND)
    assert_color(r.read_color(), san_bits(first), "first frame")
    hist, valid = r.read_temporal_history()
    assert valid
    r.clear_color(CLEAR)
    r.draw_geometry(S.scene_data_struct(*cams[1], w, h), opaque, transparent)
    before, depth = r.read_color(), r.read_depth()
    m = GL.temporal_reproject(viewproj(cams[0], w, h), viewproj(cams[1], w, h))
    r.temporal_resolve(m, BLEND)
    want = TR.run_ref(before, depth, hist, m, BLEND)
    assert 0.5 < want["valid"].mean() < 1.0, "most of the frame reprojects, a strip at one side does not"
    assert (want["color"] != before).any()
    assert_color(r.read_color(), want["color"], "atrium, second frame")
    assert_history(r, want["history"], (0, 0, w, h), "atrium, second frame")
    r.close()


# ---------------------------------------------------------------- 3. convergence to the supersampled frame
def test_jittered_frames_converge_to_their_mean(hip):
    """16 Halton jitters of a static camera, blend 1 / (n + 1), no clamp: the running mean.  The reproject of a static
    camera is the identity, and at 128 x 64 the identity samples the history texel itself (test_temporal_ref.py), so frame n
    leaves h_n = h16(fma(b_n, c_n - h_{n-1}, h_{n-1})), b_n = fl(1 / (n + 1)).  With M_n the exact running mean,
    e_n = h_n - M_n obeys e_n = e_{n-1} n / (n + 1) + d_n, where d_n is that step's rounding: the half store, 2^-11 V
    (2^-25 among subnormals), and the fp32 roundings of b_n, of the difference and of the fma, 2^-24 V each with |c - h| <= V
    and |o| <= V, V the largest of the pixel's 16 values (every h_n lies between the smallest and the largest of them).  So
    |e_16| <= 16 ((2^-11 + 3 * 2^-24) V + 2^-25).  Frame 0 stores c_0 itself; counting it too only widens the bound."""
    w, h, n_frames = 128, 64, 16
    pos, pitch, yaw = S.config3_camera()
    view = GL.camera_view(pos, pitch, yaw)
    _, proj, _, ambient, sun_dir, sun_color = GL.scene_data(view, w, h)
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    unjittered = r.read_color()
    frames = []
    for n in range(n_frames):
        jx, jy = GL.halton(n + 1, 2) - f32(0.5), GL.halton(n + 1, 3) - f32(0.5)
        pj = GL.jitter_projection(proj, jx, jy, w, h)
        r.clear_color(CLEAR)
        r.draw_geometry(A.scene_struct(view, pj, GL.matmul(pj, view), ambient, sun_dir, sun_color), opaque, transparent)
        frame = r.read_color()
        assert np.any(frame != unjittered, axis=-1).mean() > 0.01, f"jitter {n} ({jx}, {jy}) moves too little"
        frames.append(PR.floats(san_bits(frame)[..., :3]).astype(np.float64))
        r.temporal_resolve(ID, 1.0 / (n + 1), A.TEMPORAL_NO_CLAMP)
    got = PR.floats(r.read_color()[..., :3]).astype(np.float64)
    stack = np.stack(frames)
    top = stack.max(0)
    bound = n_frames * ((2.0 ** -11 + 3 * 2.0 ** -24) * top + 2.0 ** -25)
    err = np.abs(got - stack.mean(0))
    print(f"largest error {err.max():.6g}, largest error over bound {np.max(err / bound):.4f}")
    assert (err <= bound).all()
    assert (stack.max(0) - stack.min(0) > 0.05).mean() > 0.01, "the jittered frames disagree along the edges"
    r.close()


# ---------------------------------------------------------------- 4. when the history counts
def test_first_call_reset_and_a_changed_scissor_take_the_current_colour(hip):
    pytest.importorskip("torch")
    w, h = PLANE
    colors = [PR.random_hdr(w, h, seed=s) for s in (71, 72, 73, 74)]
    depth = TR.random_depth(w, h, seed=75)
    b = Bound(hip, colors[0], depth)
    hist, valid = b.r.read_temporal_history()
    assert not hist.any() and not valid, "no history before the first resolve"
    b.r.temporal_resolve(ID, BLEND)
    assert_color(b.read(), san_bits(colors[0]), "first call")
    assert_history(b.r, np.where(np.arange(4) < 3, san_bits(colors[0]), 0), (0, 0, w, h), "first call")
    b.upload(colors[1])
    b.r.temporal_resolve(ID, BLEND, A.TEMPORAL_RESET)
    assert_color(b.read(), san_bits(colors[1]), "RESET")
    assert b.r.read_temporal_history()[1]
    b.upload(colors[2])
    b.r.set_scissor(*ODD_SCISSOR)
    assert not b.r.read_temporal_history()[1], "another scissor: the history does not count"
    b.r.temporal_resolve(ID, BLEND)
    m_in = inside_of((h, w), ODD_SCISSOR)
    assert_color(b.read(), np.where(m_in[..., None], san_bits(colors[2]), colors[2]), "changed scissor")
    hist, valid = b.r.read_temporal_history()
    assert valid
    b.upload(colors[3])
    b.r.temporal_resolve(ID, BLEND)  # the same scissor again: now it counts
    want = TR.run_ref(colors[3], depth, hist, ID, BLEND, scissor=ODD_SCISSOR)
    assert want["valid"][m_in].all()
    assert_color(b.read(), want["color"], "same scissor again")
    b.r.set_scissor(0, 0, w, h)
    assert not b.r.read_temporal_history()[1]
    b.close()


# ---------------------------------------------------------------- 5. nothing else moves
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
    m = TR.ndc_translation(2.5, -1.25, w, h)
    r.temporal_resolve(m, BLEND)
    one = TR.run_ref(first["color"], first["depth"], None, m, BLEND, history_valid=False, scissor=scissor)
    assert_color(r.read_color(), one["color"], "first resolve under a scissor")
    r.temporal_resolve(m, BLEND)
    two = TR.run_ref(one["color"], first["depth"], one["history"], m, BLEND, scissor=scissor)
    got = r.read_color()
    assert_color(got, two["color"], "second resolve under a scissor")
    inside = inside_of((h, w), scissor)
    assert np.array_equal(got[~inside], first["color"][~inside]) and np.array_equal(got[..., 3], first["color"][..., 3])
    assert (got[inside][:, :3] != first["color"][inside][:, :3]).any()
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    assert np.array_equal(r.read_ids(), first["ids"])
    for a, plane in first["attr"].items():
        assert np.array_equal(r.read_attribute(a).view(np.uint32), plane.view(np.uint32)), a
    r.set_scissor(0, 0, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)  # a forward pass after it is what it was
    assert_color(r.read_color(), first["color"], "forward pass after a resolve")
    r.close()


# ---------------------------------------------------------------- 6. ordering
def test_a_deferred_clear_lands_before_the_pass(hip):
    w, h = 96, 64
    r = hip.create(w, h)
    depth = r.read_depth()
    r.clear_color(PATTERN)  # deferred: no pass has taken it
    r.temporal_resolve(ID, BLEND)
    cleared = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    one = TR.run_ref(cleared, depth, None, ID, BLEND, history_valid=False)
    assert_color(r.read_color(), one["color"], "clear, then resolve")
    r.clear_color(CLEAR)  # deferred again: the second resolve must blend the new clear colour with the history
    r.temporal_resolve(ID, BLEND, A.TEMPORAL_NO_CLAMP)
    cleared = np.broadcast_to(LR.store(np.array(CLEAR, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    two = TR.run_ref(cleared, depth, one["history"], ID, BLEND, TR.NO_CLAMP)
    assert not np.array_equal(two["color"], cleared) and not np.array_equal(two["color"], one["color"])
    assert_color(r.read_color(), two["color"], "second clear, then resolve")
    r.close()


def test_replayed_behind_an_overflowing_pass(hip):
    """two resolves behind a pass that overflows: both are void the first time and run once each in the replay, with the
    history roles they were given at the call (the second reads what the first wrote)"""
    w, h = 160, 96
    m = TR.ndc_translation(1.5, 0.75, w, h)
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        r.clear_color(PATTERN)
        r.temporal_resolve(ID, BLEND)  # a history to start from
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        r.temporal_resolve(m, BLEND)  # enqueued behind a pass that is still void
        r.temporal_resolve(m, BLEND, A.TEMPORAL_NO_CLAMP)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes, r.read_temporal_history())
        if caps is None:
            depth = r.read_depth()
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    hist0 = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    hist0[..., 3] = 0
    one = TR.run_ref(forward, depth, hist0, m, BLEND)
    two = TR.run_ref(one["color"], depth, one["history"], m, BLEND, TR.NO_CLAMP)
    assert_color(frames[None][0], two["color"], "forward frame, resolved twice")
    assert_color(frames[64][0], frames[None][0], "resolves behind a replayed pass")
    assert_color(frames[64][2][0], frames[None][2][0], "history behind a replayed pass")
    assert_color(frames[None][2][0], two["history"], "history")
    assert frames[64][2][1] and frames[None][2][1]


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, two resolves, then a pass that overflows: the resolves landed before the failing pass and the replay
    starts at that pass, so each is applied exactly once.  The last pass draws a third of the opaque objects and the
    transparent ones over the loaded depth, so most pixels still show what the resolves left."""
    w, h = 160, 96
    m = TR.ndc_translation(1.5, 0.75, w, h)
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        before, depth = r.read_color(), r.read_depth()
        one = TR.run_ref(before, depth, None, m, BLEND, history_valid=False)
        two = TR.run_ref(one["color"], depth, one["history"], m, BLEND)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.temporal_resolve(m, BLEND)
        r.temporal_resolve(m, BLEND)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_color(), r.get_stats().replayed_passes, r.read_temporal_history()[0])
        r.close()
    assert frames[None][1] == 0 and frames[64][1] > 0
    assert not np.array_equal(two["color"], one["color"]), "the second resolve is visible: the pass is not idempotent"
    kept = np.all(frames[None][0] == two["color"], axis=-1)
    assert 0.2 < kept.mean() < 1.0, "a good part of the frame shows the resolves, and the last pass drew over the rest"
    assert_color(frames[64][0], frames[None][0], "resolves in front of a replayed pass")
    assert_color(frames[None][2], two["history"], "history")
    assert_color(frames[64][2], two["history"], "history in front of a replayed pass")


# ---------------------------------------------------------------- 7. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color(PATTERN)
    r.temporal_resolve(ID, BLEND)
    before, (hist, valid) = r.read_color(), r.read_temporal_history()
    assert valid and hist.any()
    nan, inf = float("nan"), float("inf")
    bad_m = TR.identity()
    bad_m[2][1] = nan
    inf_m = TR.identity()
    inf_m[0][0] = inf
    bad = [dict(blend=v) for v in (0.0, -0.5, 1.5, nan, inf, -inf)] + [dict(flags=4), dict(flags=A.TEMPORAL_RESET | 8)] + \
          [dict(reproject=bad_m), dict(reproject=inf_m)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.temporal_resolve(**dict(dict(reproject=ID, blend=BLEND, flags=0), **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_temporal_resolve(r.h, None) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.temporal_resolve(ID, BLEND)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert_color(r.read_color(), before, "refused calls change nothing")
    hist2, valid2 = r.read_temporal_history()
    assert valid2 and np.array_equal(hist2, hist), "nor the history"
    r.temporal_resolve(ID, 1.0)  # the largest blend there is
    assert_color(r.read_color(), before, "blend 1 of a frame that is its own history")
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color(PATTERN)
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.temporal_resolve(ID, BLEND)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    assert not r8.read_temporal_history()[1]
    r8.close()


# ---------------------------------------------------------------- 8. the C++ host
def test_demo_taa_equals_the_python_path(tmp_path, hip):
    """svr_demo --taa: four frames, each drawn with its Halton jitter and resolved.  The Python path takes the unjittered
    scene and the flattened objects of a run without the flag, jitters with glmath (bit for bit svr_math.h's,
    test_jitter.py) and makes the same calls."""
    import test_host_cpp_temporal as HT
    frames, blend = 4, 0.25
    plain, taa = str(tmp_path / "plain"), str(tmp_path / "taa")
    p = HT.run_demo(hip.path, plain, frames=1)
    assert p.returncode == 0, p.stdout
    q = HT.run_demo(hip.path, taa, "--taa", str(blend), frames=frames)
    assert q.returncode == 0, q.stdout
    w, h = HT.W, HT.H
    scene = np.fromfile(plain + ".scene", dtype=f32)
    objects = tuple(np.fromfile(f"{plain}.{k}", dtype=A.RENDER_OBJECT_DTYPE) for k in ("opaque", "transparent"))
    view, proj = scene[0:16].reshape(4, 4), scene[16:32].reshape(4, 4)
    vp = GL.matmul(proj, view)
    assert np.array_equal(vp.reshape(16), scene[32:48])
    scenes = []
    for f in range(frames):
        pj = GL.jitter_projection(proj, GL.halton(f + 1, 2) - f32(0.5), GL.halton(f + 1, 3) - f32(0.5), w, h)
        s = scene.copy()
        s[16:32], s[32:48] = pj.reshape(16), GL.matmul(pj, view).reshape(16)
        scenes.append(s)
    assert np.array_equal(np.fromfile(taa + ".scene", dtype=f32), scenes[-1]), "the demo's last frame is drawn with the fourth jitter"
    # the same resources in the same creation order as SvrEngine::init + svr_demo (test_host_cpp.python_side), then the frames
    r = hip.create(w, h)
    white = r.create_image(S.white_1x1())
    r.create_image(np.array([[[0xAA, 0xAA, 0xAA, 0xFF]]], dtype=np.uint8))
    r.create_image(np.array([[[0, 0, 0, 0xFF]]], dtype=np.uint8))
    checker = r.create_image(S.checkerboard_32())
    nearest = r.create_sampler(**S.SAMPLER_NEAREST)
    linear = r.create_sampler(**S.SAMPLER_LINEAR)
    r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), white, linear)
    r.write_material(A.PASS_TRANSPARENT, (0.4, 0.3, 0.2, 1.0), checker, nearest)
    mesh, cube = S.MeshAsset("cubes"), S.cube_mesh()
    for prim in range(2):
        v = cube.vertices.copy()
        v["position"][:, 0] += np.float32(1.25 * prim)
        mesh.add_primitive(v["position"], v["normal"], np.stack([v["uv_x"], v["uv_y"]], axis=1), cube.indices, prim)
    r.upload_mesh(mesh.indices, mesh.vertices)
    for f in range(frames):
        r.clear_color((1, 1, 1, 1))
        r.draw_geometry(A.SvrSceneData.from_buffer_copy(scenes[f].tobytes()), *objects)
        if f == frames - 1:
            unresolved = r.read_color()
        r.temporal_resolve(GL.temporal_reproject(vp, vp) if f else ID, blend)
    want = r.read_color()
    r.close()
    got = np.fromfile(taa + ".color", dtype=np.uint16).reshape(h, w, 4)
    assert (want != unresolved).any(axis=-1).mean() > 0.01, "the resolve must matter"
    assert_color(got, want, "svr_demo --taa")
