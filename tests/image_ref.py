"""A second, independent statement of the image rules: the colour target's stores and loads (S1), the
transparent blend (S2, contract C12), mip generation (S3, C13) and the blit to the swapchain (S4, C16).

Same spirit as tests/raster_ref.py: numpy, Python integers and fractions.Fraction; nothing of the package is imported and
no library is loaded.  The rules are written from their definitions - IEEE 754 binary16 / binary32, the Vulkan blit and
UNORM rules as DESIGN.md / SURVEY.md quote them - not from the kernels' operation order.

Every function works on exact rationals and returns, per channel, the SET OF ADMISSIBLE STORED VALUES (half bit patterns
or bytes):

  * An fp32 chain is followed as a running forward error bound, as in raster_ref.py: eps = 2^-24 per rounding, times the
    magnitude rounded; input errors go through the partial derivatives; one more eps |result| for the second order.
  * AN OPERATION WHOSE EXACT RESULT IS ITSELF A BINARY32 NUMBER ADDS NOTHING (`_rounded`): a correctly rounded operation
    returns that number.  A chain that is exact throughout - dyadic weights, an identity extent, a constant colour -
    therefore has allowance 0 and its result is one value, ties included.
  * The admissible set is { store(fl32(x)) : |x - exact| <= allowance }.  The stores are monotone, so the set is every
    code between store(exact - allowance) and store(exact + allowance).
  * A pixel whose set has more than one element (in any channel) is "offered".

WRONG names a deliberately wrong variant of one rule (tests/test_image_ref.py shows that each is caught); None is the
reference."""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

EPS = Fr(1, 2 ** 24)
RGBA16F, RGBA8 = 0, 1            # colour target formats (include/svr.h: SvrColorFormat)
B8G8R8A8, R8G8B8A8 = 0, 1        # swapchain formats (include/svr.h: SvrSwapchainFormat)
WRONG = None
VARIANTS = ("blend_src_alpha", "blend_classic", "blend_unrounded_dst", "f16_rounded_once", "unorm8_truncate", "unorm8_half_up",
            "depth_test_greater", "transparent_writes_depth", "mip_coord_2i", "mip_ceil_extent", "mip_half_up", "blit_taps_floor_u",
            "blit_wrap", "blit_no_swap")
HALF_INF, HALF_MAX = 0x7c00, Fr(65504)


def is_wrong(name):
    assert name in VARIANTS
    return WRONG == name


# ---------------------------------------------------------------- S1: binary32, binary16 and UNORM8
def _floor_log2(x):
    """floor(log2 x) of a positive Fraction, exactly"""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    return e if (Fr(2) ** e if e >= 0 else Fr(1, 2 ** -e)) <= x else e - 1


def _pow2(e):
    return Fr(2 ** e) if e >= 0 else Fr(1, 2 ** -e)


def round_binary(x, precision, emin):
    """x (Fraction) rounded to nearest, ties to even, on the grid of a binary format with `precision` significand bits and
    least normal exponent emin (below 2^emin the grid is the subnormals').  No upper limit: the caller decides overflow."""
    if x == 0:
        return Fr(0)
    quantum = _pow2(max(_floor_log2(abs(x)), emin) - (precision - 1))
    return round(x / quantum) * quantum  # (round() of a Fraction: nearest integer, ties to even)


def fl32(x):
    """binary32 (the values here stay far below its overflow threshold)"""
    return round_binary(x, 24, -126)


def is_f32(x):
    d = x.denominator
    if d & (d - 1):
        return False
    n = abs(x.numerator)
    # a multiple of 2^-149 with at most 24 significant bits (the values here stay far below binary32's overflow threshold)
    return n == 0 or (d.bit_length() - 1 <= 149 and (n // (n & -n)).bit_length() <= 24)


def _rounded(value, err=Fr(0)):
    """The running bound after one more fp32 operation whose exact result (on exact operands) is `value` and whose operands
    carry the propagated error `err`: + eps |value|, unless nothing was wrong so far and the result is a binary32 number."""
    if err == 0 and is_f32(value):
        return Fr(0)
    return err + EPS * abs(value)


@functools.lru_cache(maxsize=None)
def half_value(bits):
    """binary16 load: exact.  -> Fraction, or float('inf') / float('-inf') / float('nan')"""
    bits = int(bits)
    s, e, m = bits >> 15, (bits >> 10) & 31, bits & 1023
    if e == 31:
        return float("nan") if m else (float("-inf") if s else float("inf"))
    v = Fr(m, 2 ** 24) if e == 0 else Fr(1024 + m, 1024) * _pow2(e - 15)
    return -v if s else v


def half_bits(x, negative_zero=False):
    """a Fraction on the binary16 grid (or beyond its range: infinity) -> its bit pattern"""
    s = 0x8000 if (x < 0 or (x == 0 and negative_zero)) else 0
    x = abs(x)
    if x == 0:
        return s
    if x >= 65520:  # the midpoint of 65504 and 2^16: from here on round-to-nearest gives infinity, as IEEE 754 says
        return s | HALF_INF
    e = _floor_log2(x)
    if e < -14:
        return s | int(x * 2 ** 24)
    return s | ((e + 15) << 10) | int((x / _pow2(e) - 1) * 1024)


def store_f16_one(x):
    """fp16 store of the exact value x: the fp32 value exists first (a shader's output), then it is rounded to nearest
    even to binary16 - two roundings.  A negative value that rounds to zero keeps its sign."""
    if isinstance(x, float):  # infinities pass through (no NaN is ever stored by the cases here)
        assert not math.isnan(x)
        return HALF_INF | (0x8000 if x < 0 else 0)
    y = x if is_wrong("f16_rounded_once") else fl32(x)
    if abs(y) >= 65520:
        return half_bits(y)
    return half_bits(round_binary(y, 11, -14), negative_zero=x < 0)


def _half_order(bits):
    """half bit patterns in value order (-0 just below +0)"""
    return bits if bits < 0x8000 else -(bits & 0x7fff) - 1


def _half_unorder(k):
    return k if k >= 0 else ((-k - 1) | 0x8000)


def store_f16(x, allow=Fr(0)):
    """-> frozenset of the admissible half bit patterns of a value within `allow` of x"""
    if allow == 0 or isinstance(x, float):
        return frozenset((store_f16_one(x),))
    lo, hi = _half_order(store_f16_one(x - allow)), _half_order(store_f16_one(x + allow))
    return frozenset(_half_unorder(k) for k in range(lo, hi + 1))


def _round_unorm8(y):
    """y in [0, 255] -> byte"""
    if is_wrong("unorm8_truncate"):
        return int(y)
    if is_wrong("unorm8_half_up"):
        return int(y + Fr(1, 2))
    return int(round(y))  # half to even


def store_un8_one(x):
    """UNORM8 store of the exact value x: NaN -> 0, the fp32 value clamped to [0, 1], x 255 - a binary32 product like any
    other, exact for every binary16 value (h * 255 has at most 19 significant bits) - and rounded half to even."""
    if isinstance(x, float):
        return 0 if (math.isnan(x) or x < 0) else 255
    return _round_unorm8(fl32(255 * min(max(fl32(x), 0), 1)))


def store_un8(x, allow=Fr(0)):
    """-> frozenset of the admissible bytes of a value within `allow` of x (the store is monotone)"""
    if allow == 0 or isinstance(x, float):
        return frozenset((store_un8_one(x),))
    return frozenset(range(store_un8_one(x - allow), store_un8_one(x + allow) + 1))


@functools.lru_cache(maxsize=None)
def load_un8(c):
    """UNORM8 load: the exact quotient c / 255"""
    return Fr(int(c), 255)


def load_un8_error(c):
    """what an fp32 implementation's loaded value may be off by: it multiplies by a rounded 1/255 (one rounding of the
    constant, one of the product); c / 255 is a binary32 number only for 0 and 255"""
    return Fr(0) if int(c) in (0, 255) else 2 * EPS * Fr(int(c), 255)


def half_to_un8(bits):
    """fp16 -> UNORM8 (a read-back of an RGBA16F target as bytes, the identity blit): exact throughout, one value for every
    one of the 65 536 patterns; NaN -> 0, negative -> 0, +inf -> 255"""
    (b,) = store_un8(half_value(bits))
    return b


def load(code, fmt):
    return half_value(code) if fmt == RGBA16F else load_un8(code)


def load_error(code, fmt):
    return Fr(0) if fmt == RGBA16F else load_un8_error(code)


def store(x, allow, fmt):
    return store_f16(x, allow) if fmt == RGBA16F else store_un8(x, allow)


# ---------------------------------------------------------------- S2: the transparent blend (C12)
class BlendResult:
    """sets[(y, x)] = [R, G, B, A] frozensets of admissible codes, for every pixel a transparent fragment blended into;
    every other pixel keeps its colour.  depth: the target's depth after the pass (transparent fragments write none).
    last[(y, x)] = per colour channel the (exact value, allowance) of the pixel's last blend, where no set before it had more
    than one element (for the error-over-allowance figures).  """


def blend_pass(color, depth, layers, fmt, scissor=None):
    """One pass of transparent layers over a target that holds `color` (H, W, 4 codes: half bit patterns or bytes, finite)
    and `depth` (H, W float32: the opaque depth).  layers, in submission order: (coverage (H, W) bool, z, (r, g, b, a)) with
    z and the source colour exact (Fractions or floats that are binary32 numbers; a source allowance may be given as a
    fifth element).  scissor (x, y, w, h): fragments outside it are discarded.

    Per pixel, in submission order:  rgb <- store(dst.rgb * dst.a + src.rgb), one fp32 rounding before the store;
    a <- store(src.a).  dst is the STORED texel, loaded by S1.  A fragment takes part iff its depth >= the pixel's opaque
    depth (equal passes); it writes no depth, so transparent layers do not hide one another.

    Allowance.  RGBA16F: the loads are exact, the product of two halves (22 bits) is exact inside the fused multiply-add,
    the sum is rounded once - that rounding is the rule's own, so the allowance is the source's (0 for exact sources).
    RGBA8: d = c / 255 and al = a / 255 arrive with load_un8_error each, so d * al is off by |al| dd + |d| dal; the sum's
    rounding is the rule's own; + eps |result| for the second order."""
    H, W = depth.shape
    inside = np.zeros((H, W), bool)
    sx, sy, sw, sh = scissor if scissor else (0, 0, W, H)
    inside[sy:sy + sh, sx:sx + sw] = True
    out = BlendResult()
    out.sets, out.last, out.depth = {}, {}, depth.copy()
    state = {}  # (y, x) -> per channel a list of (code, value as the next layer reads it)
    for layer in layers:
        cov, z, src = layer[0], layer[1], [Fr(v) for v in layer[2]]
        src_allow = Fr(layer[3]) if len(layer) > 3 else Fr(0)
        z32 = np.float32(z)
        passes = (z32 > out.depth) if is_wrong("depth_test_greater") else (z32 >= out.depth)
        ys, xs = np.nonzero(cov & inside & passes)
        for y, x in zip(ys.tolist(), xs.tolist()):
            st = state.get((y, x))
            if st is None:
                st = [[(int(c), load(c, fmt))] for c in color[y, x]]
            new = []
            for ch in range(3):
                codes = {}
                for dc, dv in st[ch]:
                    for ac, av in st[3]:
                        if is_wrong("blend_src_alpha"):
                            av = src[3]
                        if isinstance(dv, float) or isinstance(av, float):  # an infinity stored by an earlier layer
                            exact = dv * av
                            assert not math.isnan(exact)
                            allow = Fr(0)
                        else:
                            exact = dv * av + src[ch]
                            if is_wrong("blend_classic"):
                                exact = src[ch] * src[3] + dv * (1 - src[3])
                            allow = abs(av) * load_error(dc, fmt) + abs(dv) * load_error(ac, fmt) + src_allow
                            if allow:
                                allow += EPS * abs(exact)
                        for code in store(exact, allow, fmt):
                            codes[code] = exact if is_wrong("blend_unrounded_dst") else load(code, fmt)
                new.append(sorted(codes.items(), key=lambda kv: kv[0]))
                if len(st[ch]) == 1 and len(st[3]) == 1:
                    out.last.setdefault((y, x), [None] * 3)[ch] = (exact, allow)
                else:
                    out.last.pop((y, x), None)
            new.append([(code, load(code, fmt)) for code in sorted(store(src[3], Fr(0), fmt))])
            state[(y, x)] = new
        if is_wrong("transparent_writes_depth"):
            out.depth[ys, xs] = z32
    for key, st in state.items():
        out.sets[key] = [frozenset(code for code, _ in chan) for chan in st]
    return out


def offered_share(sets):
    """the share of pixels whose set has more than one element in some channel"""
    return sum(any(len(s) > 1 for s in chans) for chans in sets.values()) / max(1, len(sets))


# ---------------------------------------------------------------- S3: mip generation (C13)
def level_count(w, h):
    """floor(log2(max(w, h))) + 1"""
    return max(w, h).bit_length()


def level_extent(n, level):
    return max(1, -(-n // (1 << level))) if is_wrong("mip_ceil_extent") else max(1, n >> level)


def _linear_taps(n_dst, n_src, half_texel=True):
    """Destination centre i + 1/2 maps to source u = (i + 1/2) n_src / n_dst; the taps sit at floor(u - 1/2) and + 1 with
    weights 1 - f and f, f = frac(u - 1/2).  -> tap indices (unclamped) i0 and the integer weight numerators (w0, w1) over
    the denominator 2 n_dst, as int64 arrays over the destination."""
    i = np.arange(n_dst, dtype=np.int64)
    num = ((2 * i + 1) if half_texel else 2 * i) * n_src - n_dst  # (u - 1/2) * 2 n_dst
    den = 2 * n_dst
    i0 = np.floor_divide(num, den)
    w1 = num - i0 * den
    return i0, den - w1, w1, den


def downsample(img, dw, dh):
    """One LINEAR blit of an RGBA8 level (h, w, 4) to dw x dh: taps clamped to the edge, exact rational weights, the sum
    rounded to nearest, half to even.  No allowance: integers throughout."""
    sh, sw = img.shape[:2]
    half = not is_wrong("mip_coord_2i")
    i0, wx0, wx1, dx = _linear_taps(dw, sw, half)
    j0, wy0, wy1, dy = _linear_taps(dh, sh, half)
    ia, ib = np.clip(i0, 0, sw - 1), np.clip(i0 + 1, 0, sw - 1)
    ja, jb = np.clip(j0, 0, sh - 1), np.clip(j0 + 1, 0, sh - 1)
    t = img.astype(np.int64)
    wx0, wx1, wy0, wy1 = wx0[None, :, None], wx1[None, :, None], wy0[:, None, None], wy1[:, None, None]
    num = wy0 * (wx0 * t[ja][:, ia] + wx1 * t[ja][:, ib]) + wy1 * (wx0 * t[jb][:, ia] + wx1 * t[jb][:, ib])
    den = dx * dy
    q, r = np.divmod(num, den)
    up = (2 * r >= den) if is_wrong("mip_half_up") else ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))
    return (q + up).astype(np.uint8)


def mip_chain(img):
    """every level of the chain vkutil::generate_mipmaps makes: each a LINEAR blit of the one above"""
    h, w = img.shape[:2]
    chain = [np.ascontiguousarray(img, dtype=np.uint8)]
    for l in range(1, level_count(w, h)):
        chain.append(downsample(chain[-1], level_extent(w, l), level_extent(h, l)))
    return chain


# ---------------------------------------------------------------- S4: the blit to the swapchain (C16)
class BlitResult:
    """sets (dh, dw, 4) of frozensets of bytes, exact (dh, dw, 4) Fractions and allow (dh, dw, 4) Fractions, all in the
    source's channel order (R, G, B, A)."""


def _blit_axis(n_dst, n_src):
    """Per destination index: (taps i0 and i1 clamped (or wrapped by the wrong variant), the exact weight f of i1, its error
    df, the further taps the error can reach).
    The chain C16 names: ratio = fl(n_src / n_dst); u = fl(fl((i + 1/2) * ratio) - 1/2); f = fl(u - floor(u))."""
    ratio = Fr(n_src, n_dst)
    d_ratio = _rounded(ratio)
    out = []
    for i in range(n_dst):
        p = (i + Fr(1, 2)) * ratio
        dp = _rounded(p, (i + Fr(1, 2)) * d_ratio)
        u = p - Fr(1, 2)
        du = _rounded(u, dp)
        if is_wrong("blit_taps_floor_u"):
            u = p
        i0 = math.floor(u)
        f = u - i0
        df = _rounded(f, du)
        fix = (lambda k: k % n_src) if is_wrong("blit_wrap") else (lambda k: min(max(k, 0), n_src - 1))
        # where u is within du of an integer the floor may fall on either side: the filter is continuous there, and the
        # slope that applies is the neighbouring cell's, so its taps count among the differences
        reach = [fix(i0), fix(i0 + 1)] + ([fix(i0 - 1)] if f - du < 0 else []) + ([fix(i0 + 2)] if f + du >= 1 else [])
        out.append((fix(i0), fix(i0 + 1), f, df, sorted(set(reach))))
    return out


def blit(color, fmt, dw, dh):
    """LINEAR blit of a target (H, W, 4 codes, finite) to a dw x dh UNORM8 image; channels in the source's order (see
    in_destination_order).

    Value: the bilinear sum with exact rational weights over the S1-loaded texels.
    Allowance, the fp32 chain C16 names: the positions as in _blit_axis; then per channel
      top = fma(f, c10 - c00, c00), bot likewise, out = fma(g, bot - top, top):
      a difference's rounding, the weight's error times the largest difference among the taps it can reach, the loaded
      texels' own errors (RGBA8), each fma's rounding; + eps |out|.  Each step through _rounded: exact steps add nothing."""
    H, W = color.shape[:2]
    xs, ys = _blit_axis(dw, W), _blit_axis(dh, H)
    val = [[[load(c, fmt) for c in px] for px in row] for row in color.tolist()]
    err = [[[load_error(c, fmt) for c in px] for px in row] for row in color.tolist()]
    out = BlitResult()
    out.sets = np.empty((dh, dw, 4), object)
    out.exact = np.empty((dh, dw, 4), object)
    out.allow = np.empty((dh, dw, 4), object)
    cache = {}
    for j, (j0, j1, g, dg, jreach) in enumerate(ys):
        for i, (i0, i1, f, df, ireach) in enumerate(xs):
            for c in range(4):
                c00, c10, c01, c11 = val[j0][i0][c], val[j0][i1][c], val[j1][i0][c], val[j1][i1][c]
                key = (c00, c10, c01, c11, f, g, df, dg, err[j0][i0][c], err[j0][i1][c], err[j1][i0][c], err[j1][i1][c]) \
                    if (len(ireach) == 2 and len(jreach) == 2) else None
                if key is not None and key in cache:
                    exact, allow = cache[key]
                else:
                    rows = []
                    for jj, (a, b) in ((j0, (c00, c10)), (j1, (c01, c11))):
                        ea, eb = err[jj][i0][c], err[jj][i1][c]
                        diff = b - a
                        ddiff = _rounded(diff, ea + eb)
                        spread = max(abs(val[jj][p][c] - val[jj][q][c]) for p in ireach for q in ireach)
                        lerp = a + f * diff
                        rows.append((lerp, _rounded(lerp, f * ddiff + df * spread + ea)))
                    (top, dtop), (bot, dbot) = rows
                    diff = bot - top
                    ddiff = _rounded(diff, dtop + dbot)
                    spread = max(abs((1 - f) * (val[p][i0][c] - val[q][i0][c]) + f * (val[p][i1][c] - val[q][i1][c])) for p in jreach for q in jreach)
                    exact = top + g * diff
                    allow = _rounded(exact, g * ddiff + dg * spread + dtop)
                    if allow:
                        allow += EPS * abs(exact)
                    if key is not None:
                        cache[key] = (exact, allow)
                out.exact[j, i, c], out.allow[j, i, c] = exact, allow
                out.sets[j, i, c] = store_un8(exact, allow)
    return out


def in_destination_order(per_channel, dst_format):
    """(..., 4) in R, G, B, A order -> the byte order of the destination: B8G8R8A8 holds blue first"""
    if dst_format == R8G8B8A8 or is_wrong("blit_no_swap"):
        return per_channel
    return per_channel[..., [2, 1, 0, 3]]


def un8_error_ratio(byte, exact, allow):
    """how far a stored byte lies from the exact value, over what the allowance and the store's half step grant:
    |byte - 255 clamp(exact)| / (255 allow + 1/2), in (0, 1] for an admissible byte"""
    return float(abs(int(byte) - 255 * min(max(exact, 0), 1)) / (255 * allow + Fr(1, 2)))


# ---------------------------------------------------------------- S1 over arrays
def store_np(x, fmt):
    """S1's stores over a float64 array, by numpy's IEEE conversions (round to nearest even at each step): the stored
    VALUE as float64 (a half's value, or the byte).  tests/test_image_ref.py holds it to store_f16_one / store_un8_one."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    if fmt == RGBA16F:
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float64)
    return np.rint(np.clip(np.nan_to_num(x32, nan=0.0), 0, 1) * np.float32(255)).astype(np.float64)


def admissible_np(stored, exact, allow, fmt):
    """stored values (as store_np returns them) against { store(fl32(x)) : |x - exact| <= allow }: the stores are monotone,
    so membership is store(exact - allow) <= stored <= store(exact + allow).  exact, allow float64 (their own rounding,
    2^-53 relative, is nothing beside an allowance and cannot move an exact tie: exact - 0 is exact)."""
    return (store_np(exact - allow, fmt) <= stored) & (stored <= store_np(exact + allow, fmt))
