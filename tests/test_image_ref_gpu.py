"""The HIP library's stores, transparent blend, mip generation and blit against tests/image_ref.py, the independent exact
statement of those rules, with the checkers of tests/test_image_ref.py.  Nothing here comes out of the CPU
oracle.  Destinations and sources are seeded torch tensors under svr_bind_targets, so every pixel holds another value; the
depth is seeded too and loaded (SVR_DEPTH_LOAD).  The shares of offered pixels are asserted on the CPU
(tests/test_image_ref.py: they depend on the reference and the inputs alone); each test prints what it checked."""
import numpy as np
import pytest

import image_cases as IC
import image_ref as IR

A = IC.A
pytestmark = pytest.mark.gpu
f32 = np.float32
FMT_IDS = list(IC.FORMATS)
EMPTY = np.zeros(0, dtype=A.RENDER_OBJECT_DTYPE)
SWAPCHAINS = (A.SWAPCHAIN_B8G8R8A8, A.SWAPCHAIN_R8G8B8A8)


def to_device(torch, codes):
    """codes (h, w, 4) uint16 or uint8 -> a device tensor holding the same bytes"""
    return torch.from_numpy(np.ascontiguousarray(codes).view(np.int16 if codes.dtype == np.uint16 else np.uint8)).cuda()


def from_device(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


class Bound:
    """a context over caller tensors seeded with `codes` and `depth`"""

    def __init__(self, hip, torch, codes, depth, fmt):
        h, w = codes.shape[:2]
        self.torch, self.codes = torch, codes
        self.r = hip.create(w, h, fmt)
        self.color, self.depth = to_device(torch, codes), torch.from_numpy(np.ascontiguousarray(depth)).cuda()
        torch.cuda.synchronize()
        self.r.bind_targets(self.color.data_ptr(), self.depth.data_ptr())

    def reseed(self, depth):
        self.color.copy_(to_device(self.torch, self.codes))
        self.depth.copy_(self.torch.from_numpy(np.ascontiguousarray(depth)).cuda())
        self.torch.cuda.synchronize()

    def read(self):
        self.r.sync()
        return from_device(self.color, self.codes), self.depth.cpu().numpy()

    def close(self):
        self.r.sync()
        self.r.bind_targets(None, None)
        self.r.close()


# ---------------------------------------------------------------- 1. stores
def test_every_half_pattern_as_bytes(hip):
    """S1: fp16 -> UNORM8 is exact, one value per pattern (NaN -> 0, negative -> 0, +inf -> 255), through the read-back and
    through the identity blit in both channel orders - beside infinities and NaNs in the neighbouring pixels"""
    torch = pytest.importorskip("torch")
    planes = IC.half_planes()
    b = Bound(hip, torch, planes, np.zeros((256, 256), f32), A.COLOR_RGBA16F)
    try:
        want = IC.half_to_un8_table()[planes]
        got = b.r.read_color(as_rgba8=True)
        assert np.array_equal(got, want), f"read_color(as_rgba8): {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[0].tolist()}"
        for fmt in SWAPCHAINS:
            got = b.r.read_swapchain(256, 256, fmt)
            bad = got != IC.swizzle(want, fmt)
            assert not bad.any(), f"read_swapchain, format {fmt}: {int(bad.sum())} bytes differ, first at (y, x, byte) = {np.argwhere(bad)[0].tolist()}"
        assert np.array_equal(b.read()[0], planes), "reading leaves the target as it was"
    finally:
        b.close()
    print("65536 pixels x 4 channels x 3 read-backs, none offered")


# ---------------------------------------------------------------- 2. blending
@pytest.mark.parametrize("fmt", FMT_IDS)
@pytest.mark.parametrize("k_layers", [1, 3, 8, 70])
def test_blend(hip, k_layers, fmt):
    """K layers in one pass over the seeded destination: plain and under the scissor, instrumented and not, with the
    default tuning and without the tile split.  Every pixel is checked, colour and depth."""
    torch = pytest.importorskip("torch")
    f = IC.FORMATS[fmt]
    w, h = IC.BLEND_W, IC.BLEND_H
    codes, depth = IC.seeded_target(f)
    layers = IC.blend_layers(k_layers, f)
    IC.exact_source(layers)
    ref_layers = IC.reference_layers(layers, w, h)
    b = Bound(hip, torch, codes, depth, f)
    worst = [0.0]
    try:
        objs = IC.layer_objects(b.r, layers, w, h)
        b.r.set_depth_load_op(A.DEPTH_LOAD)
        for scissor in (None, IC.SCISSOR):
            ref = IR.blend_pass(codes, depth, ref_layers, f, scissor)
            b.r.set_scissor(*(scissor or (0, 0, w, h)))
            for instrumented in (0, 1):
                for tuning in (0, IC.TUNE_NO_SPLIT):
                    b.reseed(depth)
                    b.r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
                    b.r.set_option(A.OPT_TUNING, tuning)
                    b.r.draw_geometry(IC.blend_scene(), EMPTY, objs)
                    got_c, got_d = b.read()
                    n, offered = IC.check_blend(f"K={k_layers} {fmt} scissor={scissor} instrumented={instrumented} tuning={tuning}",
                                                got_c, got_d, codes, depth, ref, worst)
            print(f"K={k_layers} {fmt} scissor={scissor}: {n} pixels checked in each of 4 instances, {len(ref.sets)} blended, {offered} offered"
                  + (f", worst error / allowance {worst[0]:.3f}" if fmt == "rgba8" else ""))
        assert fmt != "rgba8" or 0.0 < worst[0] <= 1.0
        b.r.set_depth_load_op(A.DEPTH_CLEAR)
    finally:
        b.close()


# ---------------------------------------------------------------- 3. mip generation
@pytest.mark.parametrize("content", IC.MIP_CONTENTS)
def test_mip_chain(hip, content):
    r = hip.create(8, 8)
    try:
        n = sum(IC.check_mip_chain(r, w, h, content) for w, h in IC.MIP_EXTENTS)
    finally:
        r.close()
    print(f"{content}: {n} texels over {len(IC.MIP_EXTENTS)} chains, bit for bit")


# ---------------------------------------------------------------- 4. blit
@pytest.mark.parametrize("fmt", FMT_IDS)
@pytest.mark.parametrize("size", IC.BLIT_SOURCES, ids=[f"{w}x{h}" for w, h in IC.BLIT_SOURCES])
def test_blit(hip, size, fmt):
    torch = pytest.importorskip("torch")
    w, h = size
    f = IC.FORMATS[fmt]
    # the references first (exact rationals per destination pixel: seconds of Python), then the device
    plan = []
    for dw, dh in IC.blit_extents(w, h):
        key, codes = IC.blit_source_for(w, h, f, dw, dh)
        plan.append((dw, dh, key, codes, IC.blit_reference(key, codes, f, dw, dh)))
    key13, codes13 = IC.blit_source_for(w, h, f, 13, 7)
    worst, total, offered_total = [0.0], 0, 0
    for key in sorted({p[2] for p in plan}):
        codes = next(p[3] for p in plan if p[2] == key)
        b = Bound(hip, torch, codes, np.zeros((h, w), f32), f)
        try:
            for dw, dh, k, _, ref in plan:
                if k != key:
                    continue
                for dst_format in SWAPCHAINS:
                    n, offered = IC.check_blit(f"{w}x{h} {fmt} -> {dw}x{dh} format {dst_format}", b.r.read_swapchain(dw, dh, dst_format), ref, dst_format, worst)
                total, offered_total = total + n, offered_total + offered
            if key == key13:  # into a caller tensor larger than the image: the bytes behind it stay
                dw, dh = 13, 7
                dst = torch.full((dh * dw * 4 + 64,), 0x5a, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                b.r.copy_to_swapchain(dst.data_ptr(), dw, dh, A.SWAPCHAIN_R8G8B8A8)
                b.r.sync()
                out = dst.cpu().numpy()
                IC.check_blit(f"{w}x{h} {fmt} -> copy_to_swapchain {dw}x{dh}", out[:dh * dw * 4].reshape(dh, dw, 4), IC.blit_reference(key, codes, f, dw, dh),
                              A.SWAPCHAIN_R8G8B8A8)
                assert np.all(out[dh * dw * 4:] == 0x5a), "copy_to_swapchain wrote behind the image"
        finally:
            b.close()
    print(f"{w}x{h} {fmt}: {total} destination pixels, {offered_total} offered, worst error / allowance {worst[0]:.3f}")
    assert offered_total <= IC.EITHER_OR_CAP * total and 0.0 < worst[0] <= 1.0
