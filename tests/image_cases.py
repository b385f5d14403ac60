"""Seeded cases for tests/image_ref.py and the helpers that run them through a library of the svr.h ABI; shared by
tests/test_image_ref.py (CPU oracle) and tests/test_image_ref_gpu.py (HIP library).

Sources of the exact kind (blending): the identity scene (clip = position, w = 1), quads on the pixel grid with the same
colour at every corner, the 1 x 1 white texel, normal and sun along +y, ambient 0, sun colour 1, z constant per layer.
Every operation of the fragment's chain then has a binary32 number for its exact result - the interpolation's differences
are 0, 1/w = 1, the texel and the light term are 1 - so by image_ref's rule the source colour is the vertex colour and the
depth is z, allowance 0.  tests/raster_ref.py supplies the coverage (the top-left rule on the shared diagonal: every
pixel of a quad exactly once) and confirms the values; its own allowance never drops below the fixed 8 eps it grants a
trilinear filter's roundings, so `exact_source` asserts what it can say of every layer drawn: the value is exactly 1, nothing but
that floor is granted, i.e. no term that depends on the data, and the layer's own colour passes the binary32 chain unchanged."""
from fractions import Fraction as Fr

import numpy as np

import image_ref as IR
import raster_cases as RC
import raster_ref as RR
import scenarios as SC

A = RC.A
f32 = np.float32
EITHER_OR_CAP = RC.EITHER_OR_CAP
FORMATS = {"rgba16f": A.COLOR_RGBA16F, "rgba8": A.COLOR_RGBA8}
assert (A.COLOR_RGBA16F, A.COLOR_RGBA8) == (IR.RGBA16F, IR.RGBA8) and (A.SWAPCHAIN_B8G8R8A8, A.SWAPCHAIN_R8G8B8A8) == (IR.B8G8R8A8, IR.R8G8B8A8)
BOUNDS = dict(extents=(1e6, 1e6, 1e6))
TUNE_NO_SPLIT = 8  # SVR_OPT_TUNING bit 3 (csrc/svr_device.h)


# ---------------------------------------------------------------- 1. stores
def half_planes():
    """(256, 256, 4) uint16: every half pattern once per channel plane, in another order in each"""
    idx = np.arange(65536, dtype=np.uint32)
    planes = [(idx * m + o) & 0xffff for m, o in ((1, 0), (40503, 12345), (25173, 54321), (4005, 777))]
    out = np.stack(planes, axis=-1).astype(np.uint16).reshape(256, 256, 4)
    assert all(len(np.unique(out[..., c])) == 65536 for c in range(4))
    return out


_UN8_TABLE = []


def half_to_un8_table():
    """S1's byte for each of the 65 536 half patterns, made once"""
    if not _UN8_TABLE:
        _UN8_TABLE.append(np.array([IR.half_to_un8(b) for b in range(65536)], dtype=np.uint8))
    return _UN8_TABLE[0]


def swizzle(rgba, fmt):
    return rgba[..., [2, 1, 0, 3]] if fmt == A.SWAPCHAIN_B8G8R8A8 else rgba


def store_probe_floats():
    """binary32 inputs for the fp16 store: every finite half, the midpoint of every pair of neighbours (a tie) and its two
    binary32 neighbours, the overflow threshold 65520 and its neighbours, 2^-25 (the tie below the least subnormal) and
    seeded values over every binade"""
    h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = (h[:-1] + h[1:]) / 2
    mid32 = mid.astype(f32)
    assert np.all(mid32.astype(np.float64) == mid)
    rng = np.random.default_rng(811)
    rnd = (rng.uniform(1, 2, 4096) * 2.0 ** rng.integers(-30, 18, 4096)).astype(f32)
    edge = np.array([65504, 65519.996, 65520, 65520.004, 65536, 1e9, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -26, 2.0 ** -24], f32)
    pos = np.concatenate([h.astype(f32), mid32, np.nextafter(mid32, f32(0)), np.nextafter(mid32, f32(np.inf)), rnd, edge])
    return np.concatenate([pos, -pos])


def unorm8_tie_floats():
    """binary32 values c in [0, 1] whose binary32 product c * 255 is exactly k + 1/2, for even and for odd k: where
    truncation, half-up and half-to-even part ways"""
    out = []
    for k in (0, 2, 3, 4, 17, 100, 101, 126, 127, 200, 253, 254):
        c = f32((k + 0.5) / 255.0)
        for cand in (c, np.nextafter(c, f32(0)), np.nextafter(c, f32(1))):
            if f32(cand * f32(255.0)) == f32(k + 0.5):
                out.append((float(cand), k))
                break
    assert any(k % 2 == 0 for _, k in out) and any(k % 2 == 1 for _, k in out) and len(out) >= 8
    return out


# ---------------------------------------------------------------- 2. blending
BLEND_W = BLEND_H = 64
SCISSOR = (3, 5, 57, 53)
DEPTHS = (0.0, 0.125, 0.25, 0.5, 0.625, 0.75, 1.0)
MID_LOW, MID_HIGH = 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11  # half-way between two halves; the even neighbour below / above
TINY = 2.0 ** -14
CRAFT = (slice(30, 34), slice(24, 40))  # rows, columns of the crafted pixels: inside every band, across both seams


class Layer:
    def __init__(self, rect, z, rgba):
        self.rect, self.z, self.rgba = rect, float(f32(z)), tuple(float(f32(v)) for v in rgba)  # rect (x0, y0, x1, y1) in pixels


def px_quad_tris(rect, z):
    x0, y0, x1, y1 = rect
    return SC.px_quad(x0, y0, x1, y1, z)


def blend_layers(k_layers, fmt):
    """K = 1, 3, 8: quads over a band across both tile seams of the 64 x 64 target, depths below, at and above the seeded
    ones, the first at depth 1 with the half-way colours of the double-rounding pixels.  K = 70: the stack of
    test_frag_third_gpu on a 32 x 8 band (a full group of 64 fragments every second row: the ordered pass flushes
    mid-chunk), a 3-pixel sliver half way."""
    layers = []
    if k_layers == 70:
        for i in range(70):
            c = (0.004 + 0.003 * (i % 5), 0.002 * (i % 3), 0.001 * (i % 7), 1)
            layers.append(Layer((16, 28, 48, 36), 0.3 + 0.4 * (i % 11) / 11.0 if i % 4 else DEPTHS[i % 7], c))
            if i == 35:
                layers.append(Layer((25, 30, 28, 31), 0.75, (0.05, 0.0, 0.05, 1)))
        return layers
    rng = np.random.default_rng(70 + k_layers)
    for i in range(k_layers):
        rect = (18 - i % 3, 22 + i % 2, 46 + i % 4, 42 - i % 3)
        if i == 0:
            rgb = (MID_LOW, MID_HIGH, 0.5 + 2.0 ** -12) if fmt == A.COLOR_RGBA16F else (0.26, 0.13, 0.61)
            layers.append(Layer(rect, 1.0, rgb + (1,)))
        else:
            rgb = tuple(rng.integers(0, 4096, 3) / 4096.0 * (4.0 if (fmt == A.COLOR_RGBA16F and i % 3 == 2) else 1.0))
            layers.append(Layer(rect, DEPTHS[(3 + 2 * i) % 7], rgb + (1,)))
    return layers


def layer_coverage(layer, w, h):
    """the pixels of a quad, by raster_ref's rules, each exactly once"""
    cov = np.zeros((h, w), bool)
    for tri in px_quad_tris(layer.rect, layer.z):
        t = np.array(tri, np.float64)
        clip = np.zeros((3, 4), f32)
        clip[:, 0], clip[:, 1], clip[:, 2], clip[:, 3] = (t[:, 0] * 2 / w - 1).astype(f32), (t[:, 1] * 2 / h - 1).astype(f32), f32(layer.z), 1
        tr = RR.Tri(clip, np.full((3, 2), 0.5, f32), w, h)
        c = tr.coverage()
        assert not (c & cov).any(), "a pixel on the shared diagonal is covered once"
        cov |= c
    x0, y0, x1, y1 = layer.rect
    assert cov.sum() == (x1 - x0) * (y1 - y0)
    return cov


_EXACT_CHECKED = set()


def exact_source(layers, w=BLEND_W, h=BLEND_H):
    """Every layer handed in is of the exact kind (see the module text), checked per distinct (rectangle, depth, colour):
    raster_ref's texel is exactly 1, its depth z and its 1/w 1 (to the 2^-51 of its own float64 sums), and its allowance
    for the texel holds no data-dependent term - it is the fixed 8 eps of a trilinear filter's roundings.  The rest of the
    fragment chain is run here in binary32 on the layer's own colour: the interpolation fma(b2, c - c, fma(b1, c - c, c)),
    the division by the interpolated 1/w = 1, the products with the texel 1 and the light term 1 and the sum with the
    ambient term c * 0 must all return the colour's bits.  image_ref's rule (an exact operation adds nothing) then gives
    the source colour and depth allowance 0."""
    for l in layers:
        key = (l.rect, l.z, l.rgba)
        if key in _EXACT_CHECKED:
            continue
        tris = []
        for tri in px_quad_tris(l.rect, l.z):
            t = np.array(tri, np.float64)
            clip = np.zeros((3, 4), f32)
            clip[:, 0], clip[:, 1], clip[:, 2], clip[:, 3] = (t[:, 0] * 2 / w - 1).astype(f32), (t[:, 1] * 2 / h - 1).astype(f32), f32(l.z), 1
            tris.append((clip, np.full((3, 2), 0.5, f32)))
        ref = RR.render(tris, w, h, [np.full((1, 1, 4), 255, np.uint8)], (RR.LINEAR, RR.LINEAR, RR.LINEAR, 0.0, 1000.0))
        x0, y0, x1, y1 = l.rect
        assert len(ref.ys) == (x1 - x0) * (y1 - y0)
        assert np.all(ref.val["texel"] == 1.0) and np.all(np.abs(ref.val["depth"] - l.z) <= 2.0 ** -51) and np.all(np.abs(ref.val["r"] - 1.0) <= 2.0 ** -51)
        assert np.all(ref.tol["texel"] == 8 * RR.EPS), "beyond the fixed floors (4 eps a level, 4 eps the level blend) raster_ref grants the white texel nothing"
        b1, b2 = (v.astype(f32) for v in ref.tris[0].bary(ref.xs, ref.ys))
        for c in l.rgba[:3]:
            c = f32(c)
            assert np.isfinite(c)
            a = b2 * (c - c) + (b1 * (c - c) + c)   # each product is 0 and each sum c: fused or not, the same bits
            shaded = ((a / f32(1.0)) * f32(1.0)) * f32(1.0) * f32(1.0) + (a * f32(1.0)) * f32(0.0)
            assert np.all(shaded.view(np.uint32) == c.view(np.uint32)), f"colour {float(c)!r} does not pass the fragment chain unchanged"
        assert float(f32(l.z)) == l.z and 0.0 <= l.z <= 1.0
        _EXACT_CHECKED.add(key)


def reference_layers(layers, w, h):
    return [(layer_coverage(l, w, h), l.z, [Fr(v) for v in l.rgba]) for l in layers]


def layer_objects(r, layers, w, h, transparent=True):
    """one mesh object per layer, in order; white 1 x 1 texel, trilinear sampler"""
    img = r.create_image(np.full((1, 1, 4), 255, np.uint8), mipmapped=True)
    smp = r.create_sampler(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=0.0, max_lod=A.LOD_CLAMP_NONE)
    mat = r.write_material(A.PASS_TRANSPARENT if transparent else A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, smp)
    objs = []
    for l in layers:
        pos, col = [], []
        for tri in px_quad_tris(l.rect, l.z):
            for (x, y, z) in tri:
                pos.append((2.0 * x / w - 1.0, 2.0 * y / h - 1.0, z))
                col.append(l.rgba)
        mesh = r.upload_mesh(np.arange(6, dtype=np.uint32), SC.make_vertices(pos, [(0, 1, 0)] * 6, [(0.5, 0.5)] * 6, col))
        objs.append(SC.render_object(mesh, mat, 0, 6, **BOUNDS))
    return SC.objs(objs)


def blend_scene():
    return SC.identity_scene(ambient=0.0, sun=(0, 1, 0, 1))


def seeded_target(fmt, w=BLEND_W, h=BLEND_H, seed=29):
    """-> colour codes (h, w, 4) and depth (h, w) float32 for a caller-bound target.  Finite values only: zeros, half
    subnormals, values in [0, 1], negative values, values up to 65504; alphas among 0, 2^-14, 1/2, 1, 2 and 65504 (sums
    overflow to infinity, products underflow); the crafted block (CRAFT) for the double rounding: dst * dst.a = +-2^-28,
    below half a binary32 ulp of the first layer's half-way colours, depth 0 so that the first layer passes."""
    rng = np.random.default_rng(seed + fmt)
    depth = rng.choice(np.array(DEPTHS[:-1], f32), (h, w))
    if fmt == A.COLOR_RGBA8:
        color = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        kind = rng.integers(0, 4, (h, w))
        color[..., 3] = np.where(kind == 0, rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), (h, w)), color[..., 3])
        color[kind == 1, :3] = rng.choice(np.array([0, 255], np.uint8), (int((kind == 1).sum()), 3))
        return color, depth
    kind = rng.integers(0, 6, (h, w, 1))
    v = np.where(kind == 0, 0.0,
        np.where(kind == 1, rng.integers(1, 1024, (h, w, 3)) * 2.0 ** -24,
        np.where(kind == 2, rng.uniform(0, 1, (h, w, 3)),
        np.where(kind == 3, -rng.uniform(0, 4, (h, w, 3)),
        np.where(kind == 4, rng.uniform(0, 65504, (h, w, 3)), rng.uniform(0, 2, (h, w, 3)))))))
    alpha = rng.choice(np.array([0, 2.0 ** -14, 0.5, 1, 2, 65504]), (h, w, 1))
    color = np.concatenate([v, alpha], axis=-1).astype(np.float16)
    ys, xs = CRAFT
    sign = np.where((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0, 1.0, -1.0)[ys, xs]
    color[ys, xs, :3] = (sign * TINY)[..., None]
    color[ys, xs, 3] = TINY
    depth[ys, xs] = 0.0
    assert np.isfinite(color.astype(np.float32)).all()
    return color.view(np.uint16), depth


def check_blend(what, got_color, got_depth, seed_color, seed_depth, ref, ratios=None):
    """every pixel, none exempt: a blended pixel holds a member of S2's set in every channel, every other pixel its seeded
    bits; depth is the seeded depth everywhere.  -> (pixels checked, pixels offered)"""
    assert np.array_equal(got_depth.view(np.uint32), ref.depth.view(np.uint32)), f"{what}: the reference's depth moved"
    bad = got_depth.view(np.uint32) != seed_depth.view(np.uint32)
    assert not bad.any(), f"{what}: depth changed at {int(bad.sum())} pixels, first (y, x) = {np.argwhere(bad)[0].tolist()}"
    touched = np.zeros(seed_depth.shape, bool)
    for (y, x), sets in ref.sets.items():
        touched[y, x] = True
        for c in range(4):
            assert int(got_color[y, x, c]) in sets[c], \
                f"{what}: pixel (x, y) = ({x}, {y}) channel {c} holds {int(got_color[y, x, c]):#x}, admissible: {sorted(hex(v) for v in sets[c])}"
    bad = np.any(got_color != seed_color, axis=-1) & ~touched
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels outside the scissor or uncovered changed, first (y, x) = {np.argwhere(bad)[0].tolist()}"
    offered = sum(any(len(s) > 1 for s in sets) for sets in ref.sets.values())
    if ratios is not None and got_color.dtype == np.uint8:
        for (y, x), last in ref.last.items():
            for c, ea in enumerate(last):
                if ea is not None and not isinstance(ea[0], float):
                    ratios[0] = max(ratios[0], IR.un8_error_ratio(got_color[y, x, c], ea[0], ea[1]))
    return seed_depth.size, offered


# ---------------------------------------------------------------- 3. mip generation
MIP_EXTENTS = ((1, 1), (2, 1), (1, 2), (3, 3), (5, 3), (1, 7), (7, 5), (8, 4), (9, 5), (16, 16), (17, 9), (33, 17), (31, 64), (64, 1))
MIP_CONTENTS = ("random", "zeros", "full", "checker", "ties")


def mip_texture(w, h, content):
    rng = np.random.default_rng(3000 + 64 * w + h)
    if content == "random":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if content == "zeros":
        return np.zeros((h, w, 4), np.uint8)
    if content == "full":
        return np.full((h, w, 4), 255, np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    if content == "checker":  # neighbours 0 and 255: a 2:1 sum is k + 1/2
        return np.repeat((((xs + ys) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1)
    # ties: small values, so that weighted sums over the denominator 4 dw dh land on k + 1/2; the first of 256 seeded
    # draws whose level 1 holds ties with k even and with k odd - for the 5 -> 2 and 7 -> 3 weights too; only for the
    # extents of TIE_FREE, where no such draw exists, the draw with the most ties
    best, best_n = None, -1
    for _ in range(256):
        img = rng.integers(0, 7, (h, w, 4), dtype=np.uint8) * np.array([1, 2, 3, 6], np.uint8)
        even, odd = tie_counts(img)
        if even and odd:
            return img
        if even + odd > best_n:
            best, best_n = img, even + odd
    assert (w, h) in TIE_FREE, f"{w}x{h}: none of 256 draws ties on even and on odd quotients"
    return best


# extents whose level 1 cannot be k + 1/2 at all, or not on both parities: 1 x 1 has no level 1; 3 -> 1 reads the centre
# texel alone; thirds (7 -> 3) never sum to k + 1/2 on their own; every other extent of MIP_EXTENTS must tie both ways
TIE_FREE = ((1, 1), (3, 3), (1, 7))


def tie_counts(img):
    """how many of level 1's weighted sums are exactly k + 1/2 with k even, and with k odd"""
    h, w = img.shape[:2]
    t = img.astype(np.int64)
    dw, dh = max(1, w >> 1), max(1, h >> 1)
    i0, wx0, wx1, dx = IR._linear_taps(dw, w)
    j0, wy0, wy1, dy = IR._linear_taps(dh, h)
    ia, ib, ja, jb = np.clip(i0, 0, w - 1), np.clip(i0 + 1, 0, w - 1), np.clip(j0, 0, h - 1), np.clip(j0 + 1, 0, h - 1)
    X0, X1, Y0, Y1 = wx0[None, :, None], wx1[None, :, None], wy0[:, None, None], wy1[:, None, None]
    num = Y0 * (X0 * t[ja][:, ia] + X1 * t[ja][:, ib]) + Y1 * (X0 * t[jb][:, ia] + X1 * t[jb][:, ib])
    q, rem = np.divmod(num, dx * dy)
    tie = 2 * rem == dx * dy
    return int((tie & (q % 2 == 0)).sum()), int((tie & (q % 2 == 1)).sum())


def check_mip_chain(r, w, h, content):
    img = mip_texture(w, h, content)
    want = IR.mip_chain(img)
    assert len(want) == IR.level_count(w, h)
    handle = r.create_image(img, mipmapped=True)
    for l, level in enumerate(want):
        assert level.shape[:2] == (max(1, h >> l), max(1, w >> l)), f"{w}x{h} level {l}: the reference's extent {level.shape[:2]}"
        got = r.read_image_level(handle, l)
        assert got.shape == level.shape and np.array_equal(got, level), \
            f"{w}x{h} {content} level {l}: differs at {np.argwhere(got != level)[:3].tolist() if got.shape == level.shape else got.shape}"
    with np.testing.assert_raises(A.SvrError):
        r.read_image_level(handle, len(want))
    r.destroy_image(handle)
    return sum(l.shape[0] * l.shape[1] for l in want)


# ---------------------------------------------------------------- 4. blit
BLIT_SOURCES = ((37, 23), (64, 48))
BLIT_SEED = 64  # (a seed at which the offered share of every source stays under the cap: test_image_ref.py asserts it)


def blit_extents(w, h):
    """identity, 2:1, 1:2 and 3:1 of the source (floored), 64 x 64, 13 x 7, 1 x 1, 37 x 1, 1 x 23 and 111 x 69"""
    return [(w, h), (w // 2, h // 2), (2 * w, 2 * h), (w // 3, h // 3), (64, 64), (13, 7), (1, 1), (37, 1), (1, 23), (111, 69)]


def dyadic_weights(n_dst, n_src):
    """whether the axis interpolates, and all of its weights are halves, quarters, eighths or sixteenths"""
    _, _, w1, den = IR._linear_taps(n_dst, n_src)
    dens = {int(den // np.gcd(int(v), int(den))) for v in w1 if v}
    return bool(dens) and all(d in (2, 4, 8, 16) for d in dens)


def blit_source(w, h, fmt, dyadic=False, seed=None):
    """codes (h, w, 4).  RGBA16F: random halves in [-0.25, 1.25] with a block of HDR values and a block of an exact 0 / 1
    checker.  RGBA8: random bytes with a 0 / 255 checker block - except for the extents with dyadic weights
    (dyadic=True: 2:1, 1:2 and their like, see blit_source_for), where the bytes are multiples of 16 with alpha 0 or 255
    and a 3 x 3 block of arbitrary bytes.  That is a departure from "random bytes" and it is forced: under weights of
    halves and quarters a sum of arbitrary bytes is exactly k + 1/2 at a quarter of the pixels, an RGBA8 load is not exact
    (the kernels multiply by a rounded 1/255), so every such pixel is offered either way and the 1 % cap cannot hold;
    multiples of 16 keep those sums whole."""
    rng = np.random.default_rng((BLIT_SEED if seed is None else seed) + w + fmt)
    ys, xs = np.mgrid[0:h, 0:w]
    check = ((xs + ys) & 1)[4:12, 3:17]
    if fmt == A.COLOR_RGBA8:
        if dyadic:
            c = (16 * rng.integers(0, 16, (h, w, 4))).astype(np.uint8)
            c[..., 3] = 255 * rng.integers(0, 2, (h, w))
            c[14:17, 20:23] = rng.integers(0, 256, (3, 3, 4), dtype=np.uint8)
        else:
            c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        c[4:12, 3:17] = (check * 255)[..., None]
        return c
    c = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float16)
    c[14:20, 20:30] = rng.uniform(1.0, 16.0, (6, 10, 4)).astype(np.float16)
    c[4:12, 3:17] = check[..., None]
    return c.view(np.uint16)


def blit_source_for(w, h, fmt, dw, dh):
    """(key, codes) of the seeded source an extent is blitted from: one per format, and for RGBA8 a second one for the
    extents with dyadic weights in either axis"""
    dyadic = fmt == A.COLOR_RGBA8 and (dyadic_weights(dw, w) or dyadic_weights(dh, h))
    return ("seeded", w, h, dyadic), blit_source(w, h, fmt, dyadic)


_BLIT_REFS = {}


def blit_reference(key, codes, fmt, dw, dh):
    """S4 in the source's channel order, computed once per (key, extent) and left unchanged"""
    k = (key, fmt, dw, dh)
    if k not in _BLIT_REFS:
        _BLIT_REFS[k] = IR.blit(codes, fmt, dw, dh)
    return _BLIT_REFS[k]


def check_blit(what, got, ref, dst_format, worst=None):
    """got (dh, dw, 4) bytes in dst_format's order against S4: every pixel a member; -> (pixels, offered pixels)"""
    sets, exact, allow = (IR.in_destination_order(a, dst_format) for a in (ref.sets, ref.exact, ref.allow))
    dh, dw = got.shape[:2]
    assert sets.shape[:2] == (dh, dw)
    offered = 0
    for j in range(dh):
        for i in range(dw):
            for c in range(4):
                s = sets[j, i, c]
                assert int(got[j, i, c]) in s, (f"{what}: destination (x, y) = ({i}, {j}) byte {c} holds {int(got[j, i, c])}, admissible {sorted(s)}; "
                                                f"exact {float(exact[j, i, c]) * 255:.6f} / 255, allowance {float(allow[j, i, c]) * 255:.3e} / 255")
                if worst is not None:
                    worst[0] = max(worst[0], IR.un8_error_ratio(got[j, i, c], exact[j, i, c], allow[j, i, c]))
            offered += any(len(sets[j, i, c]) > 1 for c in range(4))
    return dh * dw, offered
