"""The UI overlay pass (include/svr_overlay.h) on the MI355X.

The reference is tests/native/overlay_ref.cpp (overlay_ref.py), the sequential painter of DESIGN C43-C49 that
test_overlay_ref.py pins on the CPU.  Every comparison is on the texel words, over the whole image, with no tolerance, and
the statistics are those the reference counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as g
import overlay_ref as R
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
pytestmark = pytest.mark.gpu
f32 = np.float32
EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
TUNE_NO_POLL = 16
FORMATS = [R.BGRA, R.RGBA]
KERNEL = os.path.join(g.ROOT, "simple-vk-renderer_amd", "csrc", "k_overlay.hip")


def capacities():
    text = open(KERNEL).read()
    return tuple(int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1)) for name in ("OVERLAY_CHUNK", "OVERLAY_KEPT"))


class Image:
    """an image and a list's textures in device memory"""

    def __init__(self, image, lst=None):
        import torch
        self.torch = torch
        self.h, self.w = image.shape
        self.dev = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint32).view(np.int32).copy()).cuda()
        self.tex = [torch.from_numpy(np.ascontiguousarray(t[0], dtype=np.uint8).copy()).cuda() for t in (lst["textures"] if lst else [])]
        torch.cuda.synchronize()

    def textures(self, lst):
        return [(d, t[1], t[2], t[3]) for d, t in zip(self.tex, lst["textures"])]

    def draw(self, r, fmt, lst):
        r.draw_overlay(self.dev, self.w, self.h, fmt, lst["vertices"], lst["indices"], lst["cmds"], self.textures(lst), lst["display_pos"], lst["scale"])

    def read(self, r):
        """fences the context first"""
        st = r.read_overlay_stats()
        return self.dev.cpu().numpy().view(np.uint32).copy(), {"triangles": st.triangles, "kept": st.kept, "tiles": st.tiles}


def assert_image(got, want, what):
    bad = got != want
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (y, x) = ({y}, {x}): {got[y, x]:#010x} vs {want[y, x]:#010x}")


def against_reference(hip, image, fmt, lst, what):
    pytest.importorskip("torch")
    r = hip.create(64, 64)
    dev = Image(image, lst)
    dev.draw(r, fmt, lst)
    got, stats = dev.read(r)
    r.close()
    want, count, want_stats = R.run_ref(image, fmt, lst)
    assert_image(got, want, what)
    assert np.array_equal(got[count == 0], image[count == 0])
    assert stats == want_stats, what
    return count


def textures():
    return [R.random_texture(7, 5, A.OVERLAY_TEX_RGBA8, 11), R.random_texture(7, 5, A.OVERLAY_TEX_A8, 12), R.random_texture(1, 1, A.OVERLAY_TEX_RGBA8, 13),
            R.random_texture(1, 1, A.OVERLAY_TEX_A8, 14)]


# ---------------------------------------------------------------- 1. extents, the soup, order
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(70, 45), (33, 33), (1, 1)])
def test_extents(hip, w, h, fmt):
    """edge tiles, a row width that is no multiple of four, a tile narrower than a thread's four pixels"""
    rows = R.soup(60, w, h, 3 * w + h) + R.tri((-4.0, -3.0), (w + 9.0, 0.2), (0.3, h + 7.0), col=(R.pack(255, 0, 0, 90), R.pack(0, 255, 0, 200), R.pack(0, 0, 255, 30)))
    lst = R.make_list(rows, textures=textures()[:1])
    count = against_reference(hip, R.random_image(w, h, 5), fmt, lst, f"{w} x {h}")
    assert count.max() >= 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_soup(hip, fmt):
    lst = R.make_list(R.soup(300, 96, 64, 2024), textures=textures()[:1])
    count = against_reference(hip, R.random_image(96, 64, 6), fmt, lst, "a soup of 300 triangles")
    assert count.max() >= 4


@pytest.mark.parametrize("fmt", FORMATS)
def test_order_across_waves_chunks_and_drains(hip, fmt):
    """more translucent triangles over one tile than three chunks or three kept lists hold, in distinct colours: a record
    out of place, dropped or taken twice at a wave, chunk or drain boundary changes the texels under it"""
    chunk, kept = capacities()
    n = 3 * max(chunk, kept) + 7
    rng = np.random.default_rng(99)
    rows = []
    for k in range(n):
        c = rng.uniform(10.0, 22.0, 2)
        p = c + rng.uniform(-10.0, 10.0, (3, 2))  # inside tile (0, 0)
        rows += R.tri(*[(f32(q[0]), f32(q[1])) for q in p], col=R.pack((k * 7) % 256, (k * 13 + 5) % 256, (k // 3) % 256, 60 + k % 150))
    count = against_reference(hip, R.random_image(40, 36, 8), fmt, R.make_list(rows), "order")
    assert count[:32, :32].max() > 100 and not count[32:].any() and not count[:, 32:].any()


# ---------------------------------------------------------------- 2. commands, clip rectangles, textures
def command_list(display_pos, scale):
    rows = R.soup(40, 96, 64, 77)
    rows += R.tri((-50.0, -50.0), (400.0, -50.0), (-50.0, 400.0), col=R.pack(255, 255, 255, 160), uv=((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)))
    rows += R.tri((0.0, 0.0), (96.0, 0.0), (0.0, 64.0), col=(R.pack(255, 200, 0, 255), R.pack(0, 200, 255, 100), R.pack(90, 0, 255, 10)),
                  uv=((-0.5, -0.25), (1.5, 0.0), (0.0, 1.25)))
    big, wide = 120, 123
    cmds = [((3.25, 2.75, 40.5, 30.5), 0, 0, 0, 60),        # fractional
            ((-20.0, -7.5, 50.0, 33.3), 1, 0, big, 3),      # negative, an A8 texture
            ((60.0, 50.0, 20.0, 10.0), 0, 0, big, 3),       # inverted: skipped
            ((10.0, 10.0, 80.0, 60.0), 0, 0, 0, 0),         # nothing to draw, in the middle
            ((70.0, 40.0, 5000.0, 9000.0), 2, 60, 0, 60),   # beyond the image; vertices and indices from the middle
            ((5000.0, 5000.0, 6000.0, 6000.0), 0, 0, 0, 3),  # off the image: skipped
            ((20.5, 12.5, 90.0, 55.0), 3, wide, 0, 3),      # the 1 x 1 A8 texture
            ((0.0, 0.0, 96.0, 64.0), 1, 0, wide, 3),
            ((30.2, 30.7, 30.9, 50.0), 0, 0, big, 3)]       # narrower than a pixel
    indices = list(range(126))
    return R.make_list(rows, indices=indices, cmds=cmds, textures=textures(), display_pos=display_pos, scale=scale)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("display_pos,scale", [((0.0, 0.0), (1.0, 1.0)), ((7.5, -3.25), (2.0, 2.0)), ((-2.0, 4.0), (1.5, 0.75))])
def test_commands_clip_rectangles_and_textures(hip, display_pos, scale, fmt):
    lst = command_list(display_pos, scale)
    image = R.random_image(96, 64, 9)
    count = against_reference(hip, image, fmt, lst, f"commands at {display_pos} x {scale}")
    assert count.max() >= 3 and (count == 0).any()


def test_text_over_a_blitted_frame(hip):
    pytest.importorskip("torch")
    w, h = 160, 96
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
    r.clear_color((0.1, 0.2, 0.3, 1.0))
    r.draw_geometry(scene, opaque, transparent)
    atlas = A.overlay_font(hip)[0]
    b = pkg.overlay.ListBuilder(A.overlay_font(hip))
    b.window(8, 6, 130, 64, "stats")
    for k, line in enumerate(["frametime 16.667 ms", "draw time 1.250 ms", "update time 0.031 ms", "triangles 262144", "draws 1024 (+5%) #"]):
        b.text(12, 22 + 9 * k, line, (255, 255, 255, 255))
    b.text(100.5, 70.25, "x2", (255, 255, 0, 200), 2)
    b.rect(150, 90, 30, 30, (0, 255, 0, 128))
    vertices, indices, cmds = b.arrays()
    lst = R.make_list(vertices, indices, cmds, textures=[(atlas, 96, 48, A.OVERLAY_TEX_A8)])
    dev = Image(np.zeros((h, w), np.uint32), lst)
    r.copy_to_swapchain(dev.dev.data_ptr(), w, h, R.BGRA)
    r.sync()
    frame = dev.dev.cpu().numpy().view(np.uint32).copy()
    assert len(np.unique(frame)) > 50
    dev.draw(r, R.BGRA, lst)
    got, stats = dev.read(r)
    r.close()
    want, count, want_stats = R.run_ref(frame, R.BGRA, lst)
    assert_image(got, want, "text over a blitted frame")
    assert stats == want_stats and count.max() >= 2
    assert np.array_equal(got[count == 0], frame[count == 0]) and (got != frame).sum() > 1000


# ---------------------------------------------------------------- 3. properties
def test_an_empty_list_changes_nothing(hip):
    pytest.importorskip("torch")
    image = R.random_image(70, 45, 10)
    lst = R.make_list(R.soup(30, 70, 45, 4))
    r = hip.create(64, 64)
    dev = Image(image, lst)
    st = r.read_overlay_stats()
    assert (st.triangles, st.kept, st.tiles) == (0, 0, 0)
    dev.draw(r, R.RGBA, lst)
    after, stats = dev.read(r)
    assert stats["triangles"] == 30 and stats["kept"] > 0
    none = R.make_list([], indices=[], cmds=[])
    dev.draw(r, R.RGBA, none)
    nothing = R.make_list(lst["vertices"], lst["indices"], cmds=[(R.NO_CLIP, 0, 0, 0, 0), (R.NO_CLIP, 0, 3, 6, 0)])
    dev.draw(r, R.RGBA, nothing)
    got, again = dev.read(r)
    r.close()
    assert_image(got, after, "an empty list")
    assert again == stats


# ---------------------------------------------------------------- 4. ordering against an overflowing pass
def overlays():
    first = R.make_list(R.soup(50, 160, 96, 21) + R.tri((-5.0, -5.0), (400.0, -5.0), (-5.0, 300.0), col=R.pack(255, 128, 0, 100)))
    second = R.make_list(R.soup(50, 160, 96, 22) + R.tri((170.0, 100.0), (-300.0, 100.0), (170.0, -200.0), col=R.pack(0, 128, 255, 77)))
    return first, second


@pytest.mark.parametrize("early_overlay", [False, True], ids=["behind", "one_in_front_one_behind"])
def test_replay_blends_every_overlay_once(hip, early_overlay):
    """pass, blit, overlay, fence with queues so small that the pass overflows: blit and overlay are void the first time and
    run once in the replay.  With an overlay enqueued before the overflowing pass: that one landed and is not run again."""
    pytest.importorskip("torch")
    w, h = 160, 96
    first, second = overlays()
    start = R.random_image(w, h, 12)
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        dev = Image(start, first)
        other = Image(R.random_image(w, h, 13), first)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        if early_overlay:
            other.draw(r, R.BGRA, first)  # onto an image the blit below does not write
        r.clear_color((1.0, 1.0, 1.0, 1.0))
        r.draw_geometry(scene, opaque, EMPTY)
        r.copy_to_swapchain(dev.dev.data_ptr(), w, h, R.BGRA)
        dev.draw(r, R.BGRA, second)
        got, stats = dev.read(r)
        frames[caps] = (got, other.dev.cpu().numpy().view(np.uint32).copy(), stats, r.get_stats().replayed_passes, r.read_swapchain(w, h, R.BGRA))
        r.close()
    assert frames[None][3] == 0 and frames[64][3] > 0
    blitted = np.ascontiguousarray(frames[None][4]).view(np.uint32).reshape(h, w)
    want, _, want_stats = R.run_ref(blitted, R.BGRA, second)
    assert_image(frames[None][0], want, "blit and overlay, no overflow")
    assert_image(frames[64][0], frames[None][0], "blit and overlay behind a replayed pass")
    assert frames[None][2] == frames[64][2] == want_stats
    if early_overlay:
        once, _, _ = R.run_ref(R.random_image(w, h, 13), R.BGRA, first)
        assert_image(frames[None][1], once, "the overlay in front, no overflow")
        assert_image(frames[64][1], once, "the overlay in front of a replayed pass is blended once")


def test_a_deferred_clear_stays_deferred(hip):
    pytest.importorskip("torch")
    lst = R.make_list(R.soup(20, 64, 64, 30))
    r = hip.create(64, 64)
    r.clear_color((1.0, 0.0, 0.0, 1.0))  # deferred: no pass has taken it
    dev = Image(R.random_image(64, 64, 31), lst)
    dev.draw(r, R.RGBA, lst)
    got, _ = dev.read(r)
    assert_image(got, R.run_ref(R.random_image(64, 64, 31), R.RGBA, lst)[0], "overlay with a clear pending")
    red = r.read_color()
    r.close()
    assert (red == red[0, 0]).all() and red[0, 0].tolist() == [0x3c00, 0, 0, 0x3c00]


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_image_alone(hip):
    pytest.importorskip("torch")
    w, h = 40, 30
    image = R.random_image(w, h, 14)
    good = R.make_list(R.tri((1.0, 1.0), (30.0, 2.0), (4.0, 25.0)) + R.tri((5.0, 5.0), (35.0, 9.0), (9.0, 28.0)), textures=textures()[:2])
    r = hip.create(64, 64)
    dev = Image(image, good)
    L = hip.lib
    tex = (A.SvrOverlayTexture * 2)(*[A.SvrOverlayTexture(d.data_ptr(), t[1], t[2], t[3], 0) for d, t in zip(dev.tex, good["textures"])])

    def refused(needle, dst=True, width=w, height=h, fmt=R.RGBA, null_list=False, **kw):
        v, i = kw.pop("vertices", good["vertices"]), np.asarray(kw.pop("indices", good["indices"]), np.uint16)
        c = kw.pop("cmds", good["cmds"])
        if not (isinstance(c, np.ndarray) and c.dtype == A.OVERLAY_CMD_DTYPE):
            c = R.make_list(v, i, cmds=c)["cmds"]
        table = kw.pop("textures", tex)
        lst = A.SvrOverlayList(v.ctypes.data, i.ctypes.data, c.ctypes.data, C.cast(table, C.c_void_p), kw.pop("n_vertices", v.size), kw.pop("n_indices", i.size),
                               kw.pop("n_cmds", c.size), kw.pop("n_textures", 2), (C.c_float * 2)(*kw.pop("display_pos", (0.0, 0.0))),
                               (C.c_float * 2)(*kw.pop("scale", (1.0, 1.0))))
        for name in kw.pop("null", ()):
            setattr(lst, name, None)
        assert not kw
        rc = L.svr_draw_overlay(r.h, C.c_void_p(dev.dev.data_ptr()) if dst else None, width, height, fmt, None if null_list else C.byref(lst))
        assert rc == -1, needle
        text = L.svr_last_error().decode()
        assert text.startswith("svr_draw_overlay: ") and needle in text, text

    clip = R.NO_CLIP
    refused("null", dst=False)
    refused("null", null_list=True)
    refused("null array", null=("vertices",))
    refused("null array", null=("indices",))
    refused("null array", null=("cmds",))
    refused("null array", null=("textures",))
    refused("extent", width=0)
    refused("extent", height=0)
    refused("extent", width=16385)
    refused("unknown format", fmt=2)
    refused("SVR_OVERLAY_MAX_CMDS", n_cmds=A.OVERLAY_MAX_CMDS + 1)
    refused("SVR_OVERLAY_MAX_TEXTURES", n_textures=A.OVERLAY_MAX_TEXTURES + 1)
    many = np.zeros(3 * (A.OVERLAY_MAX_TRIANGLES + 1), np.uint16)
    refused("SVR_OVERLAY_MAX_TRIANGLES", indices=many, cmds=[(clip, 0, 0, 0, many.size)])
    refused("command 0: elem_count is not divisible by 3", cmds=[(clip, 0, 0, 0, 4)])
    refused("command 1: idx_offset + elem_count", cmds=[(clip, 0, 0, 0, 3), (clip, 0, 0, 3, 6)])
    refused("command 0: idx_offset + elem_count", cmds=[(clip, 0, 0, 7, 0)])
    refused("command 0: index out of range", cmds=[(clip, 0, 1, 0, 6)])
    refused("command 0: index out of range", indices=[0, 1, 2, 3, 4, 6])
    refused("command 0: index out of range", n_vertices=5)
    refused("command 0: texture", cmds=[(clip, 2, 0, 0, 6)])
    for k, (field, value) in enumerate([("texels", None), ("width", 0), ("height", 16385), ("format", 2)]):
        bad = (A.SvrOverlayTexture * 2)(*[A.SvrOverlayTexture(d.data_ptr(), t[1], t[2], t[3], 0) for d, t in zip(dev.tex, good["textures"])])
        setattr(bad[1], field, value)
        refused("texture 1", textures=bad)
    for bad in (float("nan"), float("inf")):
        refused("display_pos", display_pos=(0.0, bad))
        refused("scale", scale=(bad, 1.0))
    refused("scale", scale=(1.0, 0.0))
    refused("scale", scale=(-1.0, 1.0))
    got, stats = dev.read(r)
    assert_image(got, image, "after the refusals")
    assert stats == {"triangles": 0, "kept": 0, "tiles": 0}
    dev.draw(r, R.RGBA, good)  # and the context is as usable as before
    got, _ = dev.read(r)
    r.close()
    assert_image(got, R.run_ref(image, R.RGBA, good)[0], "after the refusals, a good list")
