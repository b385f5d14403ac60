"""The upscaled present (include/svr_upscale.h) on the MI355X.

The reference is tests/native/upscale_ref.cpp (upscale_ref.py), the scalar restatement of DESIGN C50-C54 that
test_upscale_ref.py pins on the CPU, fed the colour target the library itself holds.  Every comparison is on the bytes, over
the whole image, with no tolerance.  The identity test compares library against library (svr_copy_to_swapchain)."""
import ctypes as C
import functools

import numpy as np
import pytest

import __graft_entry__ as g
import svr_testlib as T
import upscale_ref as R

pkg = g.load_package()
A = pkg.abi
pytestmark = pytest.mark.gpu
EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
TUNE_NO_POLL = 16
GUARD = 0xA5C3A5C3


class Target:
    """a context over a colour target of the test's own making (uint16 [h, w, 4]: RGBA16F, uint8: RGBA8)"""

    def __init__(self, hip, color):
        import torch
        self.torch = torch
        h, w = color.shape[:2]
        self.color = torch.from_numpy(np.ascontiguousarray(color).view(np.int16 if color.dtype == np.uint16 else np.uint8).copy()).cuda()
        self.depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.r = hip.create(w, h, A.COLOR_RGBA16F if color.dtype == np.uint16 else A.COLOR_RGBA8)
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())

    def image(self, dw, dh, rows_before=0, rows_after=0, shift=0):
        """a device buffer of guard words with room for a dw x dh image `shift` texels behind rows_before rows -> (buffer, address)"""
        buf = self.torch.full(((rows_before + dh + rows_after) * dw + shift,), GUARD - (1 << 32), dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        return buf, buf.data_ptr() + 4 * (rows_before * dw + shift)

    def close(self):
        self.r.close()


def host(buf):
    return buf.cpu().numpy().view(np.uint32).copy()


def assert_bytes(got, want, what):
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    bad = (got != want).any(2)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} texels differ, first at (y, x) = ({y}, {x}): {got[y, x].tolist()} vs {want[y, x].tolist()}")


@functools.lru_cache(maxsize=None)
def source(kind, w, h):
    return {"random": lambda: R.random_target(w, h, 7 * w + h), "specials": lambda: R.random_target(w, h, 7 * w + h, specials=True),
            "checker": lambda: R.checker(w, h, 42), "finite": lambda: R.finite_target(w, h, 9), "random8": lambda: R.random_target8(w, h, 43)}[kind]()


@functools.lru_cache(maxsize=None)
def reference(kind, src, dst, fmt, sharpness, flags, variant=0):
    return R.run_ref(source(kind, *src), dst[0], dst[1], fmt, sharpness, flags, variant)


# ---------------------------------------------------------------- 1. the extents
KINDS = ["random", "random", "specials", "random", "random", "random", "checker", "random"]
SHARPNESS = [0.5, 0.0, 1.0, 0.5, 1.0, 0.0, 0.5, 1.0]
CASES = [(kind, src, dst, (R.BGRA, R.RGBA)[k % 2], sharpness) for k, ((src, dst), kind, sharpness) in enumerate(zip(R.EXTENTS, KINDS, SHARPNESS))]


@pytest.mark.parametrize("flags", [0, R.NO_SHARPEN], ids=["sharpened", "no_sharpen"])
@pytest.mark.parametrize("kind,src,dst,fmt,sharpness", CASES, ids=[f"{c[1][0]}x{c[1][1]}_to_{c[2][0]}x{c[2][1]}" for c in CASES])
def test_extents_against_the_restatement(hip, kind, src, dst, fmt, sharpness, flags):
    pytest.importorskip("torch")
    color = source(kind, *src)
    if kind == "checker":  # the clamp and the border are really exercised
        for variant in (4, 6):
            assert (reference(kind, src, dst, fmt, sharpness, 0) != reference(kind, src, dst, fmt, sharpness, 0, variant)).any(), R.WRONG_VARIANTS[variant]
    t = Target(hip, color)
    held = t.r.read_color()
    assert np.array_equal(held, color)  # what the library holds is what the restatement is fed
    buf, at = t.image(*dst)
    t.r.upscale_to_swapchain(at, dst[0], dst[1], fmt, sharpness, flags)
    t.r.sync()
    got = host(buf).view(np.uint8).reshape(dst[1], dst[0], 4)
    read = t.r.read_upscaled(dst[0], dst[1], fmt, sharpness, flags)
    t.close()
    want = reference(kind, src, dst, fmt, sharpness, flags)
    assert_bytes(got, want, f"{src} -> {dst}")
    assert_bytes(read, want, f"{src} -> {dst}, svr_read_upscaled")


@pytest.mark.parametrize("flags", [0, R.NO_SHARPEN], ids=["sharpened", "no_sharpen"])
def test_rgba8_colour_target(hip, flags):
    pytest.importorskip("torch")
    src, dst = (37, 23), (61, 45)
    t = Target(hip, source("random8", *src))
    assert np.array_equal(t.r.read_color(), source("random8", *src))
    buf, at = t.image(*dst)
    t.r.upscale_to_swapchain(buf, dst[0], dst[1], R.RGBA, 0.5, flags)  # the tensor itself
    t.r.sync()
    got = host(buf).view(np.uint8).reshape(dst[1], dst[0], 4)
    t.close()
    assert_bytes(got, reference("random8", src, dst, R.RGBA, 0.5, flags), "RGBA8 target")


# ---------------------------------------------------------------- 2. library against library
@pytest.mark.parametrize("fmt", [R.BGRA, R.RGBA])
def test_identity_without_sharpen_is_the_blit(hip, fmt):
    pytest.importorskip("torch")
    w, h = 33, 17
    t = Target(hip, source("finite", w, h))
    up, up_at = t.image(w, h)
    blit, blit_at = t.image(w, h)
    t.r.upscale_to_swapchain(up_at, w, h, fmt, 0.5, R.NO_SHARPEN)
    t.r.copy_to_swapchain(blit_at, w, h, fmt)
    t.r.sync()
    a, b = host(up), host(blit)
    t.close()
    assert np.array_equal(a, b) and len(np.unique(a)) > 100


# ---------------------------------------------------------------- 3. no byte outside the image
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_guard_rows_keep_their_bits(hip, shift):
    """an odd destination width and a start `shift` texels off 16 bytes: every row begins at another alignment, so both
    store paths run and the one-texel path ends rows"""
    pytest.importorskip("torch")
    src, dst = (37, 23), (61, 45)
    t = Target(hip, source("specials", *src))
    buf, at = t.image(dst[0], dst[1], rows_before=3, rows_after=3, shift=shift)
    t.r.upscale_to_swapchain(at, dst[0], dst[1], R.BGRA, 1.0, 0)
    t.r.sync()
    words = host(buf)
    t.close()
    first = 3 * dst[0] + shift
    assert (words[:first] == GUARD).all() and (words[first + dst[0] * dst[1]:] == GUARD).all()
    assert words[first + dst[0] * dst[1]:].size == 3 * dst[0]
    assert_bytes(words[first:first + dst[0] * dst[1]].view(np.uint8), reference("specials", src, dst, R.BGRA, 1.0, 0), f"shift {shift}")


# ---------------------------------------------------------------- 4. ordering
def test_a_deferred_clear_runs_first(hip):
    pytest.importorskip("torch")
    import torch
    r = hip.create(20, 12)
    r.clear_color((0.25, 0.5, 0.75, 1.0))  # deferred: no pass has taken it
    dst = torch.zeros((31, 50), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.upscale_to_swapchain(dst, 50, 31, R.RGBA, 0.5, 0)
    r.sync()
    got = host(dst).view(np.uint8).reshape(31, 50, 4)
    held = r.read_color()
    r.close()
    assert (got == np.array([64, 128, 191, 255], np.uint8)).all()
    assert_bytes(got, R.run_ref(held, 50, 31, R.RGBA, 0.5, 0), "clear, then upscale")


def test_replay_behind_an_overflowing_pass(hip):
    """pass, upscale, fence with queues so small that the pass overflows: the upscale is void the first time (status 1 at
    that point), runs again in the replay and reports 2; the image is the one without overflow"""
    pytest.importorskip("torch")
    import torch
    w, h, dw, dh = 96, 54, 160, 90
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        dst = torch.full((dh, dw), 0x11111111, dtype=torch.int32, device="cuda")
        status = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.clear_color((1.0, 1.0, 1.0, 1.0))
        r.draw_geometry(scene, opaque, EMPTY)
        r.set_present_status(status.data_ptr())
        r.upscale_to_swapchain(dst, dw, dh, R.BGRA, 0.5, 0)
        r.set_present_status(0)
        r.sync()
        frames[caps] = (host(dst).view(np.uint8).reshape(dh, dw, 4), status.cpu().numpy().tolist(), r.get_stats().replayed_passes, r.read_color())
        r.close()
    assert frames[None][2] == 0 and frames[64][2] > 0
    assert frames[None][1] == [0, 77, 77, 77] and frames[64][1] == [2, 77, 77, 77]
    assert np.array_equal(frames[None][3], frames[64][3])
    assert_bytes(frames[None][0], R.run_ref(frames[None][3], dw, dh, R.BGRA, 0.5, 0), "no overflow")
    assert_bytes(frames[64][0], frames[None][0], "behind a replayed pass")
    assert len(np.unique(frames[None][0].view(np.uint32))) > 50


# ---------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing(hip):
    pytest.importorskip("torch")
    import torch
    w, h, dw, dh = 20, 12, 50, 31
    r = hip.create(w, h)
    L = hip.lib
    dst = torch.full((dh, dw), 0x22222222, dtype=torch.int32, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.clear_color((0.25, 0.5, 0.75, 1.0))  # stays deferred through every refusal
    r.set_present_status(status.data_ptr())
    good = A.SvrUpscalePass(0.5, 0)

    def refused(code, needle, ctx=True, p=good, at=True, width=dw, height=dh, fmt=R.RGBA):
        rc = L.svr_upscale_to_swapchain(r.h if ctx else None, C.byref(p) if p is not None else None, C.c_void_p(dst.data_ptr()) if at else None, width, height, fmt)
        text = L.svr_last_error().decode()
        assert rc == code and text.startswith("svr_upscale_to_swapchain: ") and needle in text, (rc, text)

    refused(-1, "null", ctx=False)
    refused(-1, "null", p=None)
    refused(-1, "null", at=False)
    for bad in (float("nan"), float("inf"), -0.125, 1.5):
        refused(-1, "sharpness", p=A.SvrUpscalePass(bad, 0))
    refused(-1, "unknown flag bits", p=A.SvrUpscalePass(0.5, 2))
    refused(-1, "unknown flag bits", p=A.SvrUpscalePass(0.5, 0x80000001))
    refused(-1, "unknown format", fmt=2)
    refused(-1, "extent", width=16385)
    refused(-1, "extent", height=16385)
    refused(-1, "extent", width=0)
    refused(-5, "smaller", width=w - 1)
    refused(-5, "smaller", height=h - 1)
    r.set_row_interleave(2, 1)
    refused(-5, "svr_set_row_interleave")
    r.set_row_interleave(1, 0)
    small = np.zeros((dh, dw, 4), np.uint8)
    assert L.svr_read_upscaled(r.h, C.byref(good), dw, dh, R.RGBA, small.ctypes.data, small.nbytes - 1) == -1
    assert b"svr_read_upscaled: buffer too small" in L.svr_last_error() and not small.any()
    assert L.svr_read_upscaled(r.h, None, dw, dh, R.RGBA, small.ctypes.data, small.nbytes) == -1
    assert L.svr_read_upscaled(r.h, C.byref(good), w - 1, dh, R.RGBA, small.ctypes.data, small.nbytes) == -5
    r.sync()  # (the fence runs the deferred clear; nothing else was enqueued)
    assert (host(dst) == 0x22222222).all() and status.cpu().numpy().tolist() == [77]
    r.clear_color((0.25, 0.5, 0.75, 1.0))
    r.upscale_to_swapchain(dst, dw, dh, R.RGBA, 0.5, 0)  # and the context is as usable as before
    r.sync()
    got = host(dst).view(np.uint8).reshape(dh, dw, 4)
    r.close()
    assert (got == np.array([64, 128, 191, 255], np.uint8)).all() and status.cpu().numpy().tolist() == [0]
