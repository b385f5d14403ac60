"""Chains of passes without a fence between them: every frame of the chain against the oracle bit for bit, the order
with the caller's own stream work on both sides of a pass, overflow replays inside a chain, two contexts side by side,
and SVR_OPT_KERNEL_TIMING level 1, whose tile kernel stamps the clock itself.  Needs a real MI355X.

The two "scenes" are the atrium of svr_testlib from two cameras (inside a column: many clipped triangles; from the
gallery: few), at 96x54 and 128x72: the oracle renders each once per size.  The passes keep to the stream arrangement
they had, so no frame is compared at a large size; what SPLIT_TILES_MAX does select is which workgroups of the tile
kernel stamp its end for level 1 (all of them up to 4096 tiles, every eighth above), and no option forces the sampled
form at a small size — with a dozen workgroups it would not be a measurement — so the level-1 test also runs one
target of 65 x 65 tiles."""
import functools
import math

import numpy as np
import pytest

import __graft_entry__ as g
import svr_testlib as T

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu

SIZES = [(96, 54), (128, 72)]
CAMS = (((2.5, 1.0, -5.5), 0.2, 1.0), ((30.0, 8.0, 9.7), -0.3, 3.0))
CLEAR = (0.25, 0.5, 0.75, 1.0)  # exact in fp16
N_PASSES = 12


@functools.lru_cache(maxsize=None)
def reference(w, h, cam):
    """The oracle's frame (colour bits, depth) of camera `cam` over CLEAR."""
    r, scene, opaque, transparent = T.setup_sponza(T.load_oracle(), w, h, lod=8, tex_size=64, camera=CAMS[cam])
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    r.sync()
    out = (r.read_color().copy(), r.read_depth().copy())
    r.close()
    return out


def make_context(hip, w, h):
    r, scene0, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64, camera=CAMS[0])
    scenes = (scene0, S.scene_data_struct(*CAMS[1], w, h))
    return r, scenes, opaque, transparent


def targets(torch, dev, w, h):
    t = torch.zeros((h, w, 4), dtype=torch.float16, device=dev), torch.zeros((h, w), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)  # (made on the default stream, used on another)
    return t


def check_frames(snaps, order, w, h, what):
    for i, (c, d) in enumerate(snaps):
        ref_c, ref_d = reference(w, h, order[i])
        T.assert_images_identical(c.cpu().numpy().view(np.uint16), ref_c, f"{what}: colour of pass {i}")
        T.assert_images_identical(d.cpu().numpy(), ref_d, f"{what}: depth of pass {i}")


def chain(torch, r, scenes, opaque, transparent, tgts, order, stream, caps_at=None, fence_after=None):
    """N_PASSES passes on `stream` without a fence, pass i of camera order[i] into tgts[i % len(tgts)]; behind each pass
    the caller copies the target on the same stream, as a caller that hands frames on would.  caps_at: the pass in front
    of which the internal queues are made tiny (SVR_OPT_QUEUE_CAPS); fence_after: the pass behind which the caller fences
    (svr_sync) before it copies."""
    snaps = []
    with torch.cuda.stream(stream):
        for i in range(N_PASSES):
            color, depth = tgts[i % len(tgts)]
            if len(tgts) > 1 or i == 0:
                r.bind_targets(color.data_ptr(), depth.data_ptr())
            if caps_at == i:
                r.set_option(A.OPT_QUEUE_CAPS, 64)
            r.clear_color(CLEAR)
            r.draw_geometry(scenes[order[i]], opaque, transparent)
            if fence_after == i:
                r.sync()
            snaps.append((color.clone(), depth.clone()))
    return snaps


@pytest.mark.parametrize("n_targets", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_twelve_unfenced_passes(hip, size, n_targets):
    """A tile kernel that overtakes its own stage 1 or the tile kernel in front of it shows as a frame of the wrong scene
    or a torn one."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    w, h = size
    r, scenes, opaque, transparent = make_context(hip, w, h)
    stream = torch.cuda.Stream(device=dev)
    r.set_stream(stream.cuda_stream)
    tgts = [targets(torch, dev, w, h) for _ in range(n_targets)]
    order = [i & 1 for i in range(N_PASSES)]
    snaps = chain(torch, r, scenes, opaque, transparent, tgts, order, stream)
    stream.synchronize()
    check_frames(snaps, order, w, h, f"{w}x{h}, {n_targets} target(s)")
    r.sync()
    assert r.get_stats().replayed_passes == 0
    r.bind_targets(None, None)
    r.close()


@pytest.mark.parametrize("size", SIZES)
def test_caller_stream_order_on_both_sides_of_a_pass(hip, size):
    """The caller's fill of the target in front of a pass (no svr_clear_color: nothing deferred) is what the pass draws
    over, and the caller's copy behind it, with no synchronisation, holds the finished frame; again after svr_set_stream
    to a second stream."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    w, h = size
    r, scenes, opaque, transparent = make_context(hip, w, h)
    color, depth = targets(torch, dev, w, h)
    fill = torch.tensor(CLEAR, dtype=torch.float16, device=dev).expand(h, w, 4).contiguous()
    torch.cuda.synchronize(dev)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    snaps, order = [], []
    for k, stream in enumerate(streams):
        r.set_stream(stream.cuda_stream)
        r.bind_targets(color.data_ptr(), depth.data_ptr())
        with torch.cuda.stream(stream):
            for cam in (k, 1 - k, k):
                color.zero_()                 # (a stale fill shows as black where the frame is uncovered or blended)
                color.copy_(fill)
                r.draw_geometry(scenes[cam], opaque, transparent)
                snaps.append((color.clone(), depth.clone()))
                order.append(cam)
        stream.synchronize()
    check_frames(snaps, order, w, h, f"{w}x{h} caller order")
    r.sync()
    r.bind_targets(None, None)
    r.close()


@pytest.mark.parametrize("caps_at", [0, 6])
@pytest.mark.parametrize("size", SIZES)
def test_overflow_replay_inside_the_chain_is_invisible(hip, size, caps_at):
    """The internal queues tiny from the first pass on, or from the middle of the chain on: the pass overflows, it and the
    passes behind it are void and are replayed in order.  The caller fences three passes behind the overflowing one, in
    the middle of the chain: the copy it takes there shows whether the replay kept the order of the frames in between,
    and the queues have grown by then, so every later copy is the oracle's frame again."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    w, h = size
    r, scenes, opaque, transparent = make_context(hip, w, h)
    stream = torch.cuda.Stream(device=dev)
    r.set_stream(stream.cuda_stream)
    tgt = targets(torch, dev, w, h)
    order = [i & 1 for i in range(N_PASSES)]
    fence = caps_at + 3
    snaps = chain(torch, r, scenes, opaque, transparent, [tgt], order, stream, caps_at=caps_at, fence_after=fence)
    r.sync()
    stats = r.get_stats()
    assert stats.replayed_passes >= 1
    # the copies the caller enqueued between the passes are not in the library's log (replayed_passes tells
    # such a caller): what must hold is the target after a fence, every copy taken before the overflowing pass, and every
    # copy from the mid-chain fence on
    color, depth = tgt
    ref_c, ref_d = reference(w, h, order[-1])
    T.assert_images_identical(color.cpu().numpy().view(np.uint16), ref_c, f"{w}x{h} caps at {caps_at}: final colour")
    T.assert_images_identical(depth.cpu().numpy(), ref_d, f"{w}x{h} caps at {caps_at}: final depth")
    check_frames(snaps[:caps_at], order, w, h, f"{w}x{h} caps at {caps_at}, before the overflow")
    check_frames(snaps[fence:], order[fence:], w, h, f"{w}x{h} caps at {caps_at}, from the fence behind pass {fence} on")
    r.bind_targets(None, None)
    r.close()


def test_two_contexts_in_one_process(hip):
    """Each context brings its own internal stream: twelve unfenced passes in each, enqueued alternately."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    ctxs = []
    for (w, h) in SIZES:
        r, scenes, opaque, transparent = make_context(hip, w, h)
        stream = torch.cuda.Stream(device=dev)
        r.set_stream(stream.cuda_stream)
        color, depth = targets(torch, dev, w, h)
        r.bind_targets(color.data_ptr(), depth.data_ptr())
        ctxs.append((r, scenes, opaque, transparent, stream, color, depth, w, h, []))
    order = [i & 1 for i in range(N_PASSES)]
    for i in range(N_PASSES):
        for (r, scenes, opaque, transparent, stream, color, depth, w, h, snaps) in ctxs:
            with torch.cuda.stream(stream):
                r.clear_color(CLEAR)
                r.draw_geometry(scenes[order[i]], opaque, transparent)
                snaps.append((color.clone(), depth.clone()))
    for (r, scenes, opaque, transparent, stream, color, depth, w, h, snaps) in ctxs:
        stream.synchronize()
        check_frames(snaps, order, w, h, f"context {w}x{h}")
        r.sync()
        r.bind_targets(None, None)
        r.close()


# Level 1 against level 2 on the parent of the change that took level 1's start event away (both levels by events there),
# twelve-pass means, three repetitions per size on one MI355X: level 2 above level 1 by 4.35 / 5.35 / 5.10 us at 96x54 and
# 5.08 / 5.21 / 4.96 us at 128x72 (level 2's two hipEventRecord packets bracket the launch gaps as well).  The margin is
# the largest of these, 5.35 us, plus as much again for the spread between runs and for the ends the kernel's own stamps
# leave out (dispatch to first workgroup, last workgroup to completion signal).  With the stamps: 5.9-7.1 us.
# At the large size (the parent at 3840x2160, more than SPLIT_TILES_MAX tiles like 2080x2080): 4.04 / 5.01 / 4.84 us, inside
# the same figure.  Level 2's interval contains level 1's in every pass (its event records stand outside the launch), so
# level 1 may not read above level 2 either: the two means are taken over different passes of the same frames, whose
# spread between repetitions (under 0.5 us in the figures above) is far below the distance between the levels.
LEVEL_MARGIN_MS = 2 * 0.00535
LARGE = (2080, 2080)  # 65 x 65 = 4225 tiles: above SPLIT_TILES_MAX, where every eighth workgroup stamps the kernel's end


@pytest.mark.parametrize("size", SIZES + [LARGE])
def test_level1_tile_time(hip, size):
    w, h = size
    r, scenes, opaque, transparent = make_context(hip, w, h)

    def frames(level):
        r.set_option(A.OPT_KERNEL_TIMING, level)
        st = r.get_stats()
        assert st.timed_passes == 0  # setting the option resets the averages
        for i in range(N_PASSES):
            r.clear_color(CLEAR)
            r.draw_geometry(scenes[i & 1], opaque, transparent)
        r.sync()
        return r.get_stats()

    frames(0)  # warm
    st1 = frames(1)
    st2 = frames(2)
    print(f"{w}x{h}: level 1 tile_ms {st1.tile_ms:.5f} over {st1.timed_passes} passes, level 2 {st2.tile_ms:.5f} over {st2.timed_passes}")
    assert st1.timed_passes == N_PASSES and st2.timed_passes == N_PASSES
    assert math.isfinite(st1.tile_ms) and st1.tile_ms > 0.0
    assert st1.tile_ms <= st2.tile_ms
    assert st2.tile_ms - st1.tile_ms <= LEVEL_MARGIN_MS
    r.set_option(A.OPT_KERNEL_TIMING, 0)
    st = r.get_stats()
    assert st.timed_passes == 0
    r.close()
