"""The upscaled present's restatement (tests/native/upscale_ref.cpp, DESIGN C50-C54) pinned on the CPU: known answers
(constant images, identity, the anti-ringing range), an independent float64 statement in numpy with a derived allowance, and
the six wrong variants, each told apart on a named input.  tests/test_upscale_gpu.py then compares the library against the
restatement bit for bit."""
import numpy as np
import pytest

import upscale_ref as R

f32 = np.float32
EPS = 2.0 ** -24  # half an ulp, relative: one fp32 rounding


def un8_of(values):
    """un8 of float32 values in float64 arithmetic: 255 v has at most 32 significant bits, so the product is exact"""
    return np.rint(np.clip(values.astype(np.float64), 0.0, 1.0).astype(f32).astype(np.float64) * 255.0)


def sat(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v < 1, v, f32(1)), f32(0)).astype(f32)


# ---------------------------------------------------------------- known answers
def constant8(values, w, h):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = np.asarray(values, np.uint8)
    return img


ALL_VALUES = [tuple(range(k, k + 4)) for k in range(0, 256, 4)]
SOME_VALUES = [(0, 1, 2, 63), (64, 127, 128, 129), (191, 253, 254, 255)]


@pytest.mark.parametrize("flags", [0, R.NO_SHARPEN], ids=["sharpened", "no_sharpen"])
@pytest.mark.parametrize("src,dst", R.EXTENTS, ids=[f"{s[0]}x{s[1]}_to_{d[0]}x{d[1]}" for s, d in R.EXTENTS])
def test_constant_image_stays_constant(src, dst, flags):
    """the filter's weights do not sum to 1 exactly in fp32; the anti-ringing clamp makes P the constant itself, and the
    sharpen of five equal values is the value to two roundings: every byte is the source's.  All 256 values, four per image, one per
    channel; twelve at the two largest destinations."""
    for k, values in enumerate(SOME_VALUES if dst[0] * dst[1] > 20000 else ALL_VALUES):
        got = R.run_ref(constant8(values, *src), dst[0], dst[1], R.RGBA, sharpness=(0.0, 0.5, 1.0)[k % 3], flags=flags)
        assert (got == np.asarray(values, np.uint8)).all(), (values, src, dst)


def test_constant_half_image_stays_constant():
    values = np.array([37, 128, 200, 255]) / 255.0
    img = np.empty((23, 37, 4), np.uint16)
    img[...] = R.halves(values)
    for flags in (0, R.NO_SHARPEN):
        got = R.run_ref(img, 61, 45, R.BGRA, flags=flags)
        assert (got == np.array([200, 128, 37, 255], np.uint8)).all()


@pytest.mark.parametrize("fmt", [R.BGRA, R.RGBA])
def test_identity_without_sharpen_is_the_saturated_source(fmt):
    """t = 0 on both axes: w = (-0, 1, 0, -0), every fma adds a zero, P = s(x0, y0)"""
    img = R.random_target(33, 17, 5, specials=True)
    got = R.run_ref(img, 33, 17, fmt, flags=R.NO_SHARPEN)
    want = un8_of(sat(R.floats(img))).astype(np.uint8)
    if fmt == R.BGRA:
        want = want[..., [2, 1, 0, 3]]
    assert np.array_equal(got, want)
    img8 = R.random_target8(33, 17, 6)
    assert np.array_equal(R.run_ref(img8, 33, 17, R.RGBA, flags=R.NO_SHARPEN), img8)


def step_edges(w, h):
    img = np.zeros((h, w, 4), f32)
    img[:, w // 2:, :] = 1.0
    img[h // 2:, :, 1] = 1.0 - img[h // 2:, :, 1]
    img[..., 2] = np.where(np.add.outer(np.arange(h), np.arange(w)) % 5 < 2, 0.2, 0.8)
    img[..., 3] = np.where(np.arange(w) % 3 == 0, 0.9, 0.05)[None, :]
    return R.halves(img)


def central_range(img, dw, dh):
    """per output texel and channel, the smallest and largest of the four central texels (C52), from C51 restated in numpy"""
    h, w = img.shape[:2]
    s = sat(R.floats(img))

    def first(n_src, n_dst):
        u = (np.arange(n_dst).astype(f32) + f32(0.5)) * (f32(n_src) / f32(n_dst)) - f32(0.5)
        x0 = np.floor(u).astype(int)
        return np.clip(x0, 0, n_src - 1), np.clip(x0 + 1, 0, n_src - 1)

    xa, xb = first(w, dw)
    ya, yb = first(h, dh)
    taps = np.stack([s[ya][:, xa], s[ya][:, xb], s[yb][:, xa], s[yb][:, xb]])
    return taps.min(0), taps.max(0)


def test_anti_ringing_keeps_every_output_inside_its_central_texels():
    img = step_edges(24, 18)
    lo, hi = central_range(img, 61, 45)
    good = R.run_ref(img, 61, 45, R.RGBA, flags=R.NO_SHARPEN).astype(np.float64)
    assert (good >= un8_of(lo)).all() and (good <= un8_of(hi)).all()
    assert (un8_of(lo) < good).any() and (good < un8_of(hi)).any()  # and it interpolates
    ringing = R.run_ref(img, 61, 45, R.RGBA, flags=R.NO_SHARPEN, variant=4).astype(np.float64)
    outside = (ringing < un8_of(lo)) | (ringing > un8_of(hi))
    assert outside.mean() > 0.02, "variant 4 must overshoot on the same image"


# ---------------------------------------------------------------- the independent float64 statement
def axis64(n_src, n_dst):
    """C51 as the contract defines it (fp32, numpy's), then the textbook Catmull-Rom polynomials in float64 -> (tap indices
    [n_dst, 4] clamped, weights [n_dst, 4], the two central indices)"""
    u = (np.arange(n_dst).astype(f32) + f32(0.5)) * (f32(n_src) / f32(n_dst)) - f32(0.5)
    fl = np.floor(u)
    t = (u - fl).astype(f32).astype(np.float64)
    x0 = fl.astype(int)
    w = np.stack([(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2], 1)
    idx = np.clip(x0[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, w, np.clip(x0, 0, n_src - 1), np.clip(x0 + 1, 0, n_src - 1)


# The allowance, to first order in EPS = 2^-24 (one fp32 rounding, relative), carried along with the values:
#   weights   w0 and w2: three roundings of values at most 1, 1/2 and 1/2 in magnitude, each later multiplied by at most 1;
#             w1: one of a value up to 2.5 (multiplied by t^2 <= 1), one of t^2 (multiplied by 2.5), one of the result <= 1;
#             w3: roundings of values <= 1/2, <= 1 (times 1/2) and the result.  None exceeds 6 EPS: E_W.
#   filter    sum of w_i x_i by one product and three fmas: each rounds a partial sum, which is at most A = sum |w_i x_i|:
#             4 EPS A; the weights' errors add E_W sum |x_i|; the inputs' errors e_i add sum |w_i| e_i (the absolute weight
#             sum, at most 1.5625, is what amplifies them).
#   clamp     slope at most 1, bounds exact: P's error is p's.
#   sharpen   lo, hi: at most E = the largest of the five inputs' errors.  1 - hi: EPS.  a = min(lo, 1 - hi) / hi:
#             da = (E + EPS) / hi + a E / hi + EPS a.  peak: three roundings on the host, 3 EPS relative; k = a peak:
#             dk = |peak| da + 4 EPS |k|.  S = (n + s) + (e + w): dS = the four errors + 2 EPS S.
#             O(k) = (m + k S) / (1 + 4 k) has dO/dk = (S - 4 O) / (1 + 4 k): an error in k moves numerator and divisor
#             together, and |S - 4 m| <= 4 hi with a divisor >= 0.2 keeps the product with 1 / hi bounded.  So
#             dO = (dk |S - 4 O| + |k| dS + e_m + EPS |m + k S| + EPS (1 + 4 k) |O|) / (1 + 4 k) + EPS |O|.
#             Where hi is so small that this is not below it: both results lie within 4 hi of their m (|k| <= 0.2,
#             |S - 4 m| <= 4 hi, divisor >= 0.2), so dO <= e_m + 4 (2 hi + E) is used instead.
#   un8       the product with 255 rounds once: EPS in units of the value.
#   second order: every term above is multiplied by 1.01.
E_W = 6 * EPS


def statement64(img, dw, dh, sharpness, flags):
    """-> (values [dh, dw, 4] float64 before un8, allowance [dh, dw, 4])"""
    h, w = img.shape[:2]
    s = sat(R.floats(img)).astype(np.float64) if img.dtype == np.uint16 else (img.astype(f32) * f32(float.fromhex("0x1.010102p-8"))).astype(np.float64)
    ix, wx, xa, xb = axis64(w, dw)
    iy, wy, ya, yb = axis64(h, dh)
    taps = s[:, ix, :]  # [h, dw, 4 taps, 4 channels]
    rows = np.einsum("ik,yikc->yic", wx, taps)
    e_rows = 4 * EPS * np.einsum("ik,yikc->yic", np.abs(wx), taps) + E_W * taps.sum(2)
    vt, et = rows[iy], e_rows[iy]  # [dh, 4 taps, dw, 4 channels]
    p = np.einsum("jk,jkic->jic", wy, vt)
    e_p = np.einsum("jk,jkic->jic", np.abs(wy), et) + 4 * EPS * np.einsum("jk,jkic->jic", np.abs(wy), np.abs(vt)) + E_W * np.abs(vt).sum(1)
    central = np.stack([s[ya][:, xa], s[ya][:, xb], s[yb][:, xa], s[yb][:, xb]])
    P = np.minimum(np.maximum(p, central.min(0)), central.max(0))
    if flags & R.NO_SHARPEN:
        return P, 1.01 * (e_p + EPS)
    jn, js = np.clip(np.arange(dh) - 1, 0, dh - 1), np.clip(np.arange(dh) + 1, 0, dh - 1)
    iw, ie = np.clip(np.arange(dw) - 1, 0, dw - 1), np.clip(np.arange(dw) + 1, 0, dw - 1)
    m, n, so, e, we = P[..., :3], P[jn][..., :3], P[js][..., :3], P[:, ie, :3], P[:, iw, :3]
    e_m, errs = e_p[..., :3], [e_p[jn][..., :3], e_p[js][..., :3], e_p[:, ie, :3], e_p[:, iw, :3]]
    E = np.maximum.reduce([e_m] + errs)
    lo, hi = np.minimum.reduce([m, n, so, e, we]), np.maximum.reduce([m, n, so, e, we])
    peak = -1.0 / (8.0 - 3.0 * float(f32(sharpness)))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(hi > 0, np.minimum(lo, 1 - hi) / hi, 0.0)
        k = a * peak
        S = (n + so) + (e + we)
        den = 1 + 4 * k
        O = (m + k * S) / den
        da = (E + EPS) / hi + a * E / hi + EPS * a
        dk = abs(peak) * da + 4 * EPS * np.abs(k)
        dS = sum(errs) + 2 * EPS * S
        dO = (dk * np.abs(S - 4 * O) + np.abs(k) * dS + e_m + EPS * np.abs(m + k * S) + EPS * den * np.abs(O)) / den + EPS * np.abs(O)
    coarse = e_m + 4 * (2 * hi + E)
    dO = np.where(np.isfinite(dO) & (dO < coarse), dO, coarse)
    return np.concatenate([O, P[..., 3:]], 2), 1.01 * (np.concatenate([dO, e_p[..., 3:]], 2) + EPS)


STATEMENT_CASES = [("random", (37, 23), (61, 45), 0.5, 0), ("random", (37, 23), (61, 45), 1.0, R.NO_SHARPEN), ("random", (16, 16), (64, 64), 0.0, 0),
                   ("random", (40, 40), (40, 97), 1.0, 0), ("checker", (24, 18), (61, 45), 0.5, 0), ("random8", (37, 23), (61, 45), 0.5, 0),
                   ("specials", (33, 17), (33, 17), 1.0, 0), ("random", (2, 3), (70, 41), 0.5, 0)]


@pytest.mark.parametrize("kind,src,dst,sharpness,flags", STATEMENT_CASES, ids=[f"{c[0]}_{c[1][0]}x{c[1][1]}_to_{c[2][0]}x{c[2][1]}_{c[3]}_{c[4]}" for c in STATEMENT_CASES])
def test_against_the_float64_statement(kind, src, dst, sharpness, flags):
    """a byte equals the rounded float64 value; it may be one step off only where 255 x the float64 value lies within
    255 x the allowance of a half-integer, and at most 5 % of the values may be that close"""
    img = {"random": lambda: R.random_target(*src, 41), "checker": lambda: R.checker(*src, 42), "random8": lambda: R.random_target8(*src, 43),
           "specials": lambda: R.random_target(*src, 44, specials=True)}[kind]()
    got = R.run_ref(img, dst[0], dst[1], R.RGBA, sharpness=sharpness, flags=flags).astype(np.float64)
    value, allowance = statement64(img, dst[0], dst[1], sharpness, flags)
    v = 255.0 * np.clip(value, 0.0, 1.0)
    near = np.abs(v - (np.floor(v) + 0.5)) <= 255.0 * allowance
    exact = got == np.rint(v)
    one_step = near & ((got == np.floor(v)) | (got == np.floor(v) + 1))
    share, inside = near.mean(), ((value > 0.02) & (value < 0.98)).mean()
    print(f"{kind} {src} -> {dst}: {100 * share:.3f} % within the allowance of a half-integer, largest allowance {allowance.max():.3g}, "
          f"{100 * inside:.1f} % in (0.02, 0.98), {int((~exact).sum())} bytes one step off")
    bad = ~(exact | one_step)
    assert not bad.any(), f"{int(bad.sum())} bytes differ, first at {tuple(np.argwhere(bad)[0])}: {got[bad][0]} vs {v[bad][0]}"
    assert share <= 0.05
    assert inside >= 0.25


# ---------------------------------------------------------------- the wrong variants
@pytest.mark.parametrize("variant", sorted(R.WRONG_VARIANTS), ids=[v.replace(" ", "_") for _, v in sorted(R.WRONG_VARIANTS.items())])
def test_wrong_variants_are_told_apart(variant):
    """on the hard-edged checker plus noise, sharpened at 0.5: 24 x 18 -> 61 x 45; for variant 3, which differs from the
    contract by roundings alone (a byte moves only where a value sits on a half-integer to 1e-7), 64 x 48 -> 251 x 187, and the
    values before un8 are compared as well"""
    src, dst = ((64, 48), (251, 187)) if variant == 3 else ((24, 18), (61, 45))
    img = R.checker(*src, 42)
    good, good_values = R.run_ref(img, dst[0], dst[1], R.RGBA, sharpness=0.5, values=True)
    wrong, wrong_values = R.run_ref(img, dst[0], dst[1], R.RGBA, sharpness=0.5, variant=variant, values=True)
    differ = (good != wrong).any(2)
    values_differ = (good_values.view(np.uint32) != wrong_values.view(np.uint32)).mean()
    print(f"variant {variant} ({R.WRONG_VARIANTS[variant]}): {int(differ.sum())} of {differ.size} texels differ, {100 * values_differ:.1f} % of the values before un8")
    assert differ.any()
    assert values_differ > (0.0 if variant in (1, 6) else 0.05)
    if variant == 1:  # only where a tap is clamped at the upper edges
        assert not differ[:30, :40].any() and (differ[:, -1].any() or differ[-1, :].any())
    if variant == 6:  # only along the border
        assert not differ[1:-1, 1:-1].any()


def test_render_extent_is_the_references_truncation():
    import __graft_entry__ as g
    glmath = g.load_package().glmath
    assert glmath.render_extent(128, 72, 0.5) == (64, 36)
    assert glmath.render_extent(3840, 2160, 0.667) == (int(f32(3840) * f32(0.667)), int(f32(2160) * f32(0.667))) == (2561, 1440)
    assert glmath.render_extent(1920, 1080, 1.0) == (1920, 1080)
    assert glmath.render_extent(5, 3, 0.1) == (1, 1)
    assert glmath.render_extent(1700, 900, 0.3) == (int(f32(1700) * f32(0.3)), int(f32(900) * f32(0.3)))
