"""Auto-exposure (include/svr_exposure.h) on the MI355X.

The reference is tests/native/exposure_ref.cpp (exposure_ref.py), the scalar restatement of DESIGN C38-C42 that
test_exposure_ref.py pins on the CPU; the post pass with auto-exposure on is post_ref run with the exposure
f32(pass.exposure) * f32(state.exposure).  Both are fed the colour target the HIP library itself holds, so every
comparison here is on bit patterns, with no tolerance; the one property check against the fp64 statement takes its
allowance from test_exposure_ref.py's docstring."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g
import exposure_ref as ER
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
PLANE = (130, 67)
ODD_SCISSOR = (3, 5, 117, 59)
MEAN_ALLOW = 0.5 * np.log2(9 / 8) + 1e-6  # test_exposure_ref.py
TARGET_ALLOW = MEAN_ALLOW + np.log2(1 + 2.0 ** -23) + 2 * 2.0 ** -24 * np.log2(np.e)


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

    def load(self, color):
        """another plane into the same tensor (behind a fence)"""
        self.r.sync()
        h, w = self.shape
        self.color.copy_(self.torch.from_numpy(np.ascontiguousarray(color).view(np.int32).reshape(h, w, 2).copy()))
        self.torch.cuda.synchronize()

    def read(self):
        self.r.sync()
        h, w = self.shape
        return self.color.cpu().numpy().view(np.uint16).reshape(h, w, 4)

    def close(self):
        self.r.close()


def assert_state(got, want, what):
    got = ER.state_of(got)
    assert np.array_equal(ER.state_bits(got), ER.state_bits(want)), f"{what}: {got} vs {want}"


def assert_meter(r, color, m, prev, snap, scissor, what):
    """the state and the histogram behind one meter of `color` equal the reference's; -> the new state"""
    hist, want = ER.run_ref(color, m, prev=prev, snap=snap, scissor=scissor)
    got_hist = r.read_exposure_histogram()
    bad = np.nonzero(got_hist != hist)[0]
    assert bad.size == 0, f"{what}: bins {bad[:8].tolist()} hold {got_hist[bad[:8]].tolist()}, expected {hist[bad[:8]].tolist()}"
    assert_state(r.read_exposure(), want, what)
    return want


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{got[y, x].tolist()} vs {want[y, x].tolist()}")


def post_reference(color, state_exposure=None, scissor=None, **kw):
    p = dict(POST, **kw)
    e = f32(p["exposure"]) if state_exposure is None else f32(p["exposure"]) * f32(state_exposure)
    return PR.run_ref(color, e, p["bloom_threshold"], p["bloom_intensity"], p["bloom_levels"], p["tonemap"], scissor=scissor)["color"]


# ---------------------------------------------------------------- 1. random HDR planes
@pytest.mark.parametrize("scissor", [None, ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_random_planes(hip, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    color = ER.random_hdr(w, h, seed=61)
    m = ER.meter(low_fraction=0.05, high_fraction=0.95)
    b = Bound(hip, color)
    assert_state(b.r.read_exposure(), ER.FIRST_STATE, "before any meter")
    assert not b.r.read_exposure_histogram().any()
    if scissor:
        b.r.set_scissor(*scissor)
    b.r.meter_exposure(**m)
    st = assert_meter(b.r, color, m, None, True, scissor, f"random planes, scissor {scissor}")
    assert st["black"] > 0 and st["counted"] > 1000 and st["counted"] + st["black"] == (scissor[2] * scissor[3] if scissor else w * h)
    assert_color(b.read(), color, "the meter reads colour only")
    if scissor:  # nothing outside the scissor is read: other values out there change nothing
        x0, y0, sw, sh = scissor
        other = ER.halves(np.full((h, w, 4), 1000.0, f32))
        other[y0:y0 + sh, x0:x0 + sw] = color[y0:y0 + sh, x0:x0 + sw]
        b.load(other)
        b.r.reset_exposure()
        b.r.meter_exposure(**m)
        again = ER.state_of(b.r.read_exposure())
        assert again["meters"] == 2 and np.array_equal(ER.state_bits(dict(again, meters=1)), ER.state_bits(st))
    b.close()


# ---------------------------------------------------------------- 2. degenerate scissors
@pytest.mark.parametrize("scissor", [(7, 9, 1, 1), (8, 3, 2, 1), (5, 4, 1, 5), (129, 66, 1, 1)], ids=["1x1", "2x1", "1x5", "last_pixel"])
def test_degenerate_scissors(hip, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    color = ER.random_hdr(w, h, seed=63, specials=False, lo=-8.0, hi=8.0)
    x0, y0, sw, sh = scissor
    b = Bound(hip, color)
    b.r.set_scissor(*scissor)
    m = ER.meter(adapt=0.5)
    b.r.meter_exposure(**m)
    st = assert_meter(b.r, color, m, None, True, scissor, f"scissor {scissor}")
    assert st["counted"] == sw * sh and st["black"] == 0
    # T = 1 (or sw * sh) under a narrow window high in the ranks
    narrow = ER.meter(low_fraction=0.75, high_fraction=0.8, adapt=0.5)
    b.r.meter_exposure(**narrow)
    st = assert_meter(b.r, color, narrow, st, False, scissor, f"scissor {scissor}, narrow window")
    # T = 0: the scissor's pixels black; the window is empty and the exposure stays
    black = color.copy()
    black[y0:y0 + sh, x0:x0 + sw, :3] = 0
    b.load(black)
    b.r.meter_exposure(**m)
    after = assert_meter(b.r, black, m, st, False, scissor, f"scissor {scissor}, black")
    assert (after["counted"], after["black"], after["meters"]) == (0, sw * sh, 3)
    assert (after["exposure"], after["target"], after["mean_log2"]) == (st["exposure"], st["target"], st["mean_log2"])
    b.close()


# ---------------------------------------------------------------- 3. contention paths
def contention_plane(kind, w, h):
    if kind == "constant":  # every lane of every wave on one counter
        return ER.grey(h, w, ER.halves(0.37))
    if kind == "all_bins":  # the luminances of a row cycle through all 256 bins: the lanes of a wave are all distinct
        # green alone: L = fl(0.7152f g); g = the middle of bin i over the weight keeps L inside bin i
        centres = np.array([2.0 ** ((i >> 3) - 16) * (1 + ((i & 7) + 0.5) / 8) / 0.7152 for i in range(256)])
        centres = np.minimum(centres, 65504.0)
        out = np.zeros((h, w, 4), np.uint16)
        out[..., 1] = ER.halves(centres)[(np.arange(w)[None, :] + 5 * np.arange(h)[:, None]) % 256]
        return out
    out = np.zeros((h, w, 4), np.uint16)  # black but for one pixel
    out[h // 2, w - 3, :3] = ER.halves(2.5)
    return out


@pytest.mark.parametrize("kind", ["constant", "all_bins", "one_pixel"])
def test_contention_paths(hip, kind):
    pytest.importorskip("torch")
    w, h = 515, 9  # two chunks a row, the second one short
    color = contention_plane(kind, w, h)
    b = Bound(hip, color)
    b.r.meter_exposure(**ER.METER)
    st = assert_meter(b.r, color, ER.METER, None, True, None, kind)
    hist = b.r.read_exposure_histogram()
    if kind == "constant":
        assert (hist != 0).sum() == 1 and hist.max() == w * h
    elif kind == "all_bins":
        assert (hist != 0).sum() >= 245 and st["counted"] + st["black"] == w * h
    else:
        assert hist.sum() == 1 and st["black"] == w * h - 1
    b.close()


# ---------------------------------------------------------------- 4. more than one workgroup, more than one chunk each
def test_many_workgroups_and_chunks(hip):
    """csrc/k_exposure.hip's grid rule: a chunk is 512 pixels of one scissor row, the grid is min(chunks, 512)
    workgroups, and workgroup g walks chunks g, g + grid, ... eight at a time.  700 x 800 is 2 x 800 = 1600 chunks: 512
    workgroups of three or four chunks each, one ragged batch; 1100 x 1520 under a scissor of 1051 x 1500 is 3 x 1500 =
    4500 chunks: every workgroup takes eight or nine, so the batch of eight runs once in full and, for 404 workgroups,
    again with one chunk."""
    pytest.importorskip("torch")
    for (w, h), scissor in (((700, 800), None), ((1100, 1520), (37, 11, 1051, 1500))):
        color = ER.random_hdr(w, h, seed=67)
        b = Bound(hip, color)
        if scissor:
            b.r.set_scissor(*scissor)
        b.r.meter_exposure(**ER.METER)
        st = assert_meter(b.r, color, ER.METER, None, True, scissor, f"{w} x {h}, scissor {scissor}")
        n = scissor[2] * scissor[3] if scissor else w * h
        assert int(b.r.read_exposure_histogram().sum()) + st["black"] == n and st["counted"] + st["black"] == n
        b.close()


# ---------------------------------------------------------------- 5. a sequence
def test_a_sequence_of_meters(hip):
    pytest.importorskip("torch")
    w, h = PLANE
    planes = [ER.random_hdr(w, h, seed=71 + s, lo=-8.0 + 4 * s, hi=4 * s) for s in range(3)]
    m = ER.meter(adapt=0.25, low_fraction=0.1, high_fraction=0.9)
    b = Bound(hip, planes[0])
    st = None
    for i, p in enumerate(planes):
        if i:
            b.load(p)
        b.r.meter_exposure(**m)
        st = assert_meter(b.r, p, m, st, i == 0, None, f"meter {i + 1}")
        assert st["meters"] == i + 1
        assert (st["exposure"] == st["target"]) == (i == 0)
    b.r.reset_exposure()
    assert_state(b.r.read_exposure(), st, "a reset leaves the state")
    b.load(planes[0])
    b.r.meter_exposure(**m)
    st = assert_meter(b.r, planes[0], m, st, True, None, "the meter behind a reset snaps")
    assert st["meters"] == 4 and st["exposure"] == st["target"]
    b.r.meter_exposure(**m)
    st = assert_meter(b.r, planes[0], m, st, False, None, "and the one behind that does not")
    assert b.r.exposure_state_ptr() and b.r.exposure_state_ptr() == b.r.exposure_state_ptr()
    b.close()


# ---------------------------------------------------------------- 6. the post pass with auto-exposure
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("levels", [0, 4])
@pytest.mark.parametrize("scissor", [None, ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_post_pass_with_auto_exposure(hip, op, levels, scissor):
    pytest.importorskip("torch")
    w, h = PLANE
    # (dim enough that the metered exposure shows under every operator: with +inf texels the bloom saturates the frame)
    color = PR.random_hdr(w, h, seed=41, specials=False, top=0.0, bright=8.0)
    kw = dict(bloom_levels=levels, tonemap=OPS[op])
    b = Bound(hip, color)
    if scissor:
        b.r.set_scissor(*scissor)
    # auto on before any meter: the state's exposure is 1.0
    b.r.set_post_auto_exposure(True)
    b.r.post_pass(**dict(POST, **kw))
    off = post_reference(color, None, scissor, **kw)
    assert_color(b.read(), off, "auto on before any meter is auto off")
    b.load(color)
    m = ER.meter(key=0.25)
    b.r.meter_exposure(**m)
    b.r.post_pass(**dict(POST, **kw))
    st = assert_meter(b.r, color, m, None, True, scissor, "the meter in front of the post pass")
    assert abs(float(st["exposure"]) - 1) > 0.05
    on = post_reference(color, st["exposure"], scissor, **kw)
    assert not np.array_equal(on, off)
    assert_color(b.read(), on, f"auto on, {op}, {levels} levels, scissor {scissor}")
    b.load(color)
    b.r.set_post_auto_exposure(False)
    b.r.post_pass(**dict(POST, **kw))
    assert_color(b.read(), off, "auto off again")
    assert not b.depth.cpu().numpy().any()
    b.close()


# ---------------------------------------------------------------- 7. nothing else moves
def _planes(r):
    return {"color": r.read_color(), "depth": r.read_depth().view(np.uint32), "ids": r.read_ids(), "ambient": r.read_ambient().view(np.uint32),
            "history": r.read_temporal_history()[0],
            **{f"attr{a}": r.read_attribute(a).view(np.uint32) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}


def test_nothing_else_moves(hip):
    w, h, scissor = 160, 96, (21, 9, 100, 71)
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    r.ambient_pass(LR.inv_viewproj(scene.viewproj), 0.5, 100.0, 0.01, 1.0, 0.05, 0)
    ident = np.eye(4, dtype=f32)
    r.temporal_resolve(ident, 0.5)
    r.temporal_resolve(ident, 0.5)
    first = _planes(r)
    assert first["ambient"].any() and first["history"].any()
    r.set_scissor(*scissor)
    m = ER.meter(adapt=0.5)
    r.meter_exposure(**m)
    st = assert_meter(r, first["color"], m, None, True, scissor, "the meter under a scissor")
    r.set_scissor(0, 0, w, h)
    r.meter_exposure(**m)
    assert_meter(r, first["color"], m, st, False, None, "and over the whole target")
    after = _planes(r)
    for k, plane in first.items():
        assert np.array_equal(after[k], plane), k
    r.close()


# ---------------------------------------------------------------- 8. replay
@pytest.mark.parametrize("warm", [False, True], ids=["first_meter", "second_meter"])
def test_replayed_behind_an_overflowing_pass(hip, warm):
    """the overflow is in the pass before the meter: the meter and the auto-exposed post pass are void the first time and
    run once, in call order, in the replay.  warm: a meter before all of it has taken the snap, so the replayed one adapts
    by half and a second application would show in the exposure, not only in `meters`."""
    w, h = 160, 96
    out = {}
    for caps in (None, 64):
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        r.set_post_auto_exposure(True)
        if warm:
            r.clear_color(PATTERN)
            r.meter_exposure(**ER.METER)
            assert r.read_exposure().meters == 1
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        r.meter_exposure(**ER.meter(adapt=0.5))  # enqueued behind a pass that is still void
        r.post_pass(**POST)
        out[caps] = (r.read_color(), ER.state_of(r.read_exposure()), r.read_exposure_histogram(), r.get_stats().replayed_passes)
        if caps is None:
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert out[None][3] == 0 and out[64][3] > 0
    prev = None
    if warm:
        cleared = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
        _, prev = ER.run_ref(cleared, ER.METER)
    hist, want = ER.run_ref(forward, ER.meter(adapt=0.5), prev=prev, snap=not warm)
    for caps in (None, 64):
        color, st, got_hist, _ = out[caps]
        assert np.array_equal(ER.state_bits(st), ER.state_bits(want)), (caps, st, want)
        assert st["meters"] == (2 if warm else 1) and np.array_equal(got_hist, hist)
        assert_color(color, post_reference(forward, want["exposure"]), f"the frame, caps {caps}")
    if warm:
        assert want["exposure"] != want["target"]


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, a meter that snaps, a meter that adapts by half, then a pass that overflows: both meters landed before
    the failing pass and the replay starts at that pass, so each is applied exactly once"""
    w, h = 160, 96
    out = {}
    for caps in (None, 64):
        r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        before = r.read_color()
        r.meter_exposure(**ER.meter(key=0.7))
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the passes so far are done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.meter_exposure(**ER.meter(adapt=0.5))
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), transparent)
        out[caps] = (ER.state_of(r.read_exposure()), r.get_stats().replayed_passes)
        r.close()
    assert out[None][1] == 0 and out[64][1] > 0
    _, st = ER.run_ref(before, ER.meter(key=0.7))
    _, want = ER.run_ref(before, ER.meter(adapt=0.5), prev=st, snap=False)
    assert want["exposure"] not in (want["target"], st["exposure"]) and want["meters"] == 2
    for caps in (None, 64):
        assert np.array_equal(ER.state_bits(out[caps][0]), ER.state_bits(want)), (caps, out[caps][0], want)


# ---------------------------------------------------------------- 9. a deferred clear
def test_a_deferred_clear_lands_before_the_meter(hip):
    w, h = 96, 64
    r = hip.create(w, h)
    r.clear_color(PATTERN)  # deferred: no pass has taken it
    r.meter_exposure(**ER.METER)
    cleared = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    st = assert_meter(r, cleared, ER.METER, None, True, None, "clear, then meter")
    assert st["counted"] == w * h
    assert_color(r.read_color(), cleared, "the clear landed")
    r.close()


# ---------------------------------------------------------------- 10. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    r.clear_color(PATTERN)
    r.meter_exposure(**ER.meter(key=0.4))
    before, color = ER.state_of(r.read_exposure()), r.read_color()
    hist = r.read_exposure_histogram()
    nan, inf = float("nan"), float("inf")
    bad = [dict(key=v) for v in (0.0, -1.0, nan, inf)] + [dict(low_fraction=v) for v in (-0.1, 1.0, nan, inf)] + \
          [dict(high_fraction=v) for v in (0.0, 1.5, nan, -1.0)] + [dict(low_fraction=0.5, high_fraction=0.5), dict(low_fraction=0.6, high_fraction=0.4)] + \
          [dict(min_exposure=v) for v in (0.0, -1.0, nan, inf)] + [dict(max_exposure=v) for v in (nan, inf, 2.0 ** -11)] + \
          [dict(adapt=v) for v in (-0.1, 1.1, nan, inf)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.meter_exposure(**ER.meter(**kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_meter_exposure(r.h, None) == -1
    assert hip.lib.svr_read_exposure(r.h, None) == -1
    assert hip.lib.svr_get_exposure_state(r.h, None) == -1
    assert hip.lib.svr_debug_read_exposure_histogram(r.h, None, 1024) == -1
    small = np.zeros(255, np.uint32)
    assert hip.lib.svr_debug_read_exposure_histogram(r.h, small.ctypes.data, small.nbytes) == -1
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.meter_exposure(**ER.METER)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    assert np.array_equal(ER.state_bits(ER.state_of(r.read_exposure())), ER.state_bits(before)), "refused calls change nothing"
    assert np.array_equal(r.read_exposure_histogram(), hist) and np.array_equal(r.read_color(), color)
    # a refused meter does not take the snap either: the first accepted one of a fresh context still snaps
    r2 = hip.create(w, h)
    r2.clear_color(PATTERN)
    with pytest.raises(A.SvrError):
        r2.meter_exposure(**ER.meter(adapt=2.0))
    r2.meter_exposure(**ER.meter(adapt=0.25))
    st = r2.read_exposure()
    assert st.exposure == st.target and st.meters == 1
    r2.close()
    r.close()
    r8 = hip.create(w, h, A.COLOR_RGBA8)
    r8.clear_color(PATTERN)
    before8 = r8.read_color()
    with pytest.raises(A.SvrError, match="RGBA16F") as e:
        r8.meter_exposure(**ER.METER)
    assert e.value.code == -5
    assert np.array_equal(r8.read_color(), before8)
    assert_state(r8.read_exposure(), ER.FIRST_STATE, "an RGBA8 context's state")
    r8.close()


# ---------------------------------------------------------------- 11. the lit atrium
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


def test_lit_atrium(hip):
    w, h = 160, 96
    r, scene, opaque, _ = T.setup_sponza(hip, w, h)
    r.enable_attributes(GBUFFER)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    args = (LR.inv_viewproj(scene.viewproj),) + LR.lighting_of(scene)
    unlit = LR.run_ref(r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO), *args)
    r.light_pass(*args, lights=point_lights(65, unlit, seed=31))
    before = r.read_color()
    m = ER.meter(low_fraction=0.1, high_fraction=0.95)
    r.set_post_auto_exposure(True)
    r.meter_exposure(**m)
    r.post_pass(**POST)
    st = assert_meter(r, before, m, None, True, None, "the lit atrium")
    assert_color(r.read_color(), post_reference(before, st["exposure"]), "the lit atrium, posted with the metered exposure")
    # the property the meter is for: the exposure maps the kept pixels' geometric mean onto the key
    mean, target, T_, kept = ER.statement64(before, m)
    lum = ER.luminance64(before)
    assert kept > 5000 and not (np.abs(lum / 2.0 ** -16 - 1) < 1e-6).any()
    assert float(f32(m["min_exposure"])) < target < float(f32(m["max_exposure"])), "the clamp must not bind here"
    off = abs(np.log2(float(st["exposure"]) * 2.0 ** mean) - np.log2(float(f32(m["key"]))))
    print(f"lit atrium: exposure {float(st['exposure']):.6f}, log2(exposure * geometric mean / key) = {off:.6f} (allowed {TARGET_ALLOW:.6f})")
    assert off <= TARGET_ALLOW
    r.close()


# ---------------------------------------------------------------- 12. the C++ host
def test_cpp_host_writes_the_swapchain_python_does(tmp_path, hip):
    pytest.importorskip("torch")
    host = os.path.join(g.PKG_DIR, "host")
    w, h = 160, 90
    subprocess.run(["make", "-s"], cwd=host, check=True)

    def demo(prefix, *extra):
        return subprocess.run([os.path.join(host, "svr_demo"), "--lib", hip.path, "--width", str(w), "--height", str(h), "--frames", "1",
                               "--dump", prefix, "--deferred", "1", *extra], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)

    plain, auto = str(tmp_path / "plain"), str(tmp_path / "auto")
    p = demo(plain)
    assert p.returncode == 0, p.stdout
    q = demo(auto, "--post", "aces:4", "--auto-exposure", "0.18:1")
    assert q.returncode == 0, q.stdout
    before = np.fromfile(f"{plain}.color", dtype=np.uint16).reshape(h, w, 4)
    b = Bound(hip, before)
    b.r.set_post_auto_exposure(True)
    b.r.meter_exposure(0.18, 0.0, 1.0, 2.0 ** -10, 2.0 ** 10, 1.0)
    b.r.post_pass(1.0, 1.0, 1.0, 4, A.TONEMAP_ACES)
    want_swap = b.r.read_swapchain(w, h)
    want_color, st = b.read().copy(), b.r.read_exposure()
    b.close()
    assert np.array_equal(np.fromfile(f"{auto}.color", dtype=np.uint16).reshape(h, w, 4), want_color)
    assert np.array_equal(np.fromfile(f"{auto}.swapchain", dtype=np.uint8).reshape(h, w, 4), want_swap)
    assert not np.array_equal(np.fromfile(f"{plain}.swapchain", dtype=np.uint8).reshape(h, w, 4), want_swap)
    line = [ln for ln in q.stdout.splitlines() if ln.startswith("exposure ")]
    assert len(line) == 1, q.stdout
    words = line[0].split()
    assert words[::2] == ["exposure", "target", "mean_log2", "counted", "black", "meters"]
    assert f32(float(words[1])) == f32(st.exposure) and f32(float(words[5])) == f32(st.mean_log2)
    assert (int(words[7]), int(words[9]), int(words[11])) == (st.counted, st.black, 1)
