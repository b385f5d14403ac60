"""tests/native/post_ref.cpp, the scalar restatement of the post pass's contract (DESIGN C22-C26), checked on the CPU: its
fp16 rounding against numpy, closed forms that can be worked out by hand, the scissor as the image, an independent float64
implementation, and six deliberately wrong variants that must each be told apart."""
import numpy as np
import pytest

import post_ref as PR

f32, f64 = np.float32, np.float64


def bits_equal_or_both_nan(got, values):
    with np.errstate(over="ignore", invalid="ignore"):
        want = values.astype(np.float16)
    nan = np.isnan(values)
    g = got.view(np.float16)
    assert np.isnan(g[nan]).all() and (np.signbit(g[nan]) == np.signbit(values[nan])).all()
    bad = (got != want.view(np.uint16)) & ~nan
    assert not bad.any(), f"{int(bad.sum())} values differ, first {values[bad][0]!r}: {got[bad][0]:#06x} vs {want.view(np.uint16)[bad][0]:#06x}"


# ---------------------------------------------------------------- h16
def test_h16_is_the_identity_on_every_half():
    every = np.arange(1 << 16, dtype=np.uint16)
    values = every.view(np.float16).astype(f32)
    got = PR.h16(values)
    nan = np.isnan(values)
    assert np.array_equal(got[~nan], every[~nan])
    assert np.isnan(got[nan].view(np.float16)).all()


def test_h2f_then_h16_is_the_identity_on_every_half():
    """both directions of ref_contract.h's codec, which every restatement reads and writes its halves with, neither taken
    from numpy: every non-NaN pattern comes back as it went in; a NaN keeps its sign and its payload and comes back quiet"""
    every = np.arange(1 << 16, dtype=np.uint16)
    got = PR.roundtrip(every)
    nan = (every & 0x7fff) > 0x7c00
    assert int(nan.sum()) == 2 * 1023
    assert np.array_equal(got[~nan], every[~nan])
    assert np.array_equal(got[nan], every[nan] | 0x0200)


def test_h16_against_numpy_on_random_floats():
    rng = np.random.default_rng(1)
    any_bits = rng.integers(0, 1 << 32, 500_000, dtype=np.uint64).astype(np.uint32).view(f32)
    in_range = (rng.choice([-1.0, 1.0], 500_000) * 10.0 ** rng.uniform(-9, 5.2, 500_000)).astype(f32)
    for values in (any_bits, in_range):
        bits_equal_or_both_nan(PR.h16(values), values)


def test_h16_ties_overflow_and_subnormals():
    pos = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(f64)  # every finite half >= 0, ascending
    mid = ((pos[:-1] + pos[1:]) / 2).astype(f32)  # exact in fp32: 12 significant bits
    assert np.array_equal(mid.astype(f64), (pos[:-1] + pos[1:]) / 2)
    ties = np.concatenate([mid, -mid, np.nextafter(mid, f32(np.inf)), np.nextafter(mid, f32(0))])
    bits_equal_or_both_nan(PR.h16(ties), ties)
    got = PR.h16(mid)
    assert not (got & 1).any(), "a tie goes to the even neighbour"
    edge = np.array([65504, 65519.996, 65520, 65536, 1e10, np.inf, -65519.996, -65520, -np.inf, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25,
                     np.nextafter(f32(2.0 ** -25), f32(1)), np.nextafter(f32(2.0 ** -25), f32(0)), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24,
                     2.0 ** -14, np.nextafter(f32(2.0 ** -14), f32(0)), 1e-45, 0.0, -0.0], f32)
    bits_equal_or_both_nan(PR.h16(edge), edge)
    assert PR.h16(edge)[:6].tolist() == [0x7bff, 0x7bff, 0x7c00, 0x7c00, 0x7c00, 0x7c00]
    assert PR.h16(np.array([2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -24], f32)).tolist() == [0x0000, 0x8000, 0x0002]


# ---------------------------------------------------------------- closed forms
def tonemap32(h, op):
    """C26's operators in numpy float32 (one IEEE operation per step; the fma as an exact float64 expression rounded once)"""
    h = np.asarray(h, f32)
    if op == PR.CLAMP:
        return np.minimum(h, f32(1))
    if op == PR.REINHARD:
        return h / (f32(1) + h)
    h64 = h.astype(f64)
    fma = lambda a, b, c: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)  # exact in float64 for the magnitudes used here, rounded once
    n = h * fma(f32(2.51), h64, f32(0.03))
    d = fma(h64, fma(f32(2.43), h64, f32(0.59)), f32(0.14))
    return np.minimum(n / d, f32(1))


@pytest.mark.parametrize("levels", [1, 4, 8])
@pytest.mark.parametrize("op", [PR.CLAMP, PR.REINHARD, PR.ACES])
def test_constant_image(levels, op):
    """A constant image c = 3 with threshold 1 and exposure 1.  san(3) = 3; the box is ((3 + 3) + (3 + 3)) * 0.25 = 3; the
    bright pass 3 * 1 - 1 = 2; the blur's running sum is 0.125, 0.625, 1.375, 1.875, 2: every step exact, so B_0 = 2, and
    the box and blur of a constant 2 give 2 at every level.  The upsample of a constant is fma(t, 0, 2) = 2, so U_i = 2 +
    U_{i+1} and U_0 = 2 L.  The composite sees h = fma(intensity, 2 L, 3), one rounding, on every pixel."""
    w, h, intensity = 37, 21, 0.01
    color = np.empty((h, w, 4), np.uint16)
    color[...] = PR.halves([3.0, 3.0, 3.0, 0.625])
    ref = PR.run_ref(color, 1.0, 1.0, intensity, levels, op)
    for i, (lw, lh) in enumerate(PR.level_extents(w, h, levels)):
        assert ref["B"][i].shape == (lh, lw, 4)
        assert (ref["B"][i] == PR.halves([2.0, 2.0, 2.0, 0.0])).all()
        assert (ref["U"][i] == PR.halves([2.0 * (levels - i)] * 3 + [0.0])).all()
    hh = (f64(f32(intensity)) * (2.0 * levels) + 3.0).astype(f32)
    want = PR.h16(tonemap32(np.array([hh], f32), op))[0]
    assert (ref["color"][..., :3] == want).all()
    assert (ref["color"][..., 3] == color[..., 3]).all()


def test_single_bright_texel():
    """One texel of 1024 at (21, 21) in a black 48 x 48 image, exposure 1, threshold 0, two levels.  D_0 is 256 at (10, 10)
    and B_0 its blur: 256 * (k_x / 16) * (k_y / 16) = k_x k_y for k = {1, 4, 6, 4, 1}: integers, exact.  Every later value
    is a multiple of 2^-18 below 64, which fp32 holds exactly, so both directions of the box, the blur and the upsample
    commute and every rounding is a function of an exact value: the result is symmetric under swapping x and y."""
    color = np.zeros((48, 48, 4), np.uint16)
    color[21, 21, :3] = PR.halves(1024.0)
    ref = PR.run_ref(color, 1.0, 0.0, 1.0, 2, PR.REINHARD)
    k = np.array([1, 4, 6, 4, 1], f32)
    b0 = PR.floats(ref["B"][0])
    want = np.zeros((24, 24), f32)
    want[8:13, 8:13] = np.outer(k, k)
    for c in range(3):
        assert np.array_equal(b0[..., c], want)
    for img in (ref["B"][0], ref["B"][1], ref["U"][0], ref["color"]):
        assert np.array_equal(img, img.transpose(1, 0, 2))
    out = PR.floats(ref["color"])[..., 0]
    assert out[21, 21] > 0.99 and (out > 0).sum() > 25 * 4, "the texel itself and a halo around it"


# ---------------------------------------------------------------- the scissor is the image
def test_nothing_outside_the_scissor_is_read_or_written():
    w, h, sc = 50, 40, (3, 5, 41, 29)
    base = PR.random_hdr(w, h, seed=3)
    x0, y0, sw, sh = sc
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + sh, x0:x0 + sw] = True
    outs = []
    for fill in (None, 0x7e00, 0x7bff):
        color = base.copy()
        if fill is not None:
            color[~inside] = fill
        ref = PR.run_ref(color, 0.8, 0.5, 0.7, 4, PR.ACES, scissor=sc)
        assert np.array_equal(ref["color"][~inside], color[~inside])
        outs.append(ref["color"][inside])
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    alone = PR.run_ref(np.ascontiguousarray(base[y0:y0 + sh, x0:x0 + sw]), 0.8, 0.5, 0.7, 4, PR.ACES)
    assert np.array_equal(alone["color"].reshape(-1, 4), outs[0])
    assert np.array_equal(alone["color"][..., 3], base[y0:y0 + sh, x0:x0 + sw, 3])


# ---------------------------------------------------------------- an independent float64 implementation
def san64(v):
    return np.where(v > 0, np.minimum(v, 65504.0), 0.0)


def box64(s):
    hs, ws = s.shape[:2]
    x0, y0 = 2 * np.arange((ws + 1) // 2), 2 * np.arange((hs + 1) // 2)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    return (s[y0][:, x0] + s[y0][:, x1] + s[y1][:, x0] + s[y1][:, x1]) / 4


def blur64(s):
    k = np.array([1, 4, 6, 4, 1], f64) / 16
    hs, ws = s.shape[:2]
    xs, ys = np.arange(ws), np.arange(hs)
    hz = sum(k[j] * s[:, np.clip(xs + j - 2, 0, ws - 1)] for j in range(5))
    return sum(k[j] * hz[np.clip(ys + j - 2, 0, hs - 1)] for j in range(5))


def up64(s, w, h):
    hs, ws = s.shape[:2]
    fx, fy = np.arange(w) * 0.5 - 0.25, np.arange(h) * 0.5 - 0.25
    ix, iy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    tx, ty = (fx - ix)[None, :, None], (fy - iy)[:, None, None]
    x0, x1, y0, y1 = np.clip(ix, 0, ws - 1), np.clip(ix + 1, 0, ws - 1), np.clip(iy, 0, hs - 1), np.clip(iy + 1, 0, hs - 1)
    top = (1 - tx) * s[y0][:, x0] + tx * s[y0][:, x1]
    bot = (1 - tx) * s[y1][:, x0] + tx * s[y1][:, x1]
    return (1 - ty) * top + ty * bot


H_REL, H_ABS = 2.0 ** -11, 2.0 ** -25  # one fp16 rounding: relative in the normal range, absolute below it
F_REL = 2.0 ** -20                     # the fp32 operations between two rounding points (under twenty, 2^-24 each)


def post64(color, exposure, threshold, intensity, levels, op):
    """-> (value, allowance) of C22-C26 in float64 with no fp16 rounding point.  The allowance is carried along: every
    stage between D_0 and the composite is a combination with non-negative weights (box, blur, lerp, sum), or monotone
    with slope at most 1 (san, the clamp at 65504), so an error bound passes through the same operators as the value.  Each
    of the roundings on the way (B_0 .. B_{L-1}, U_{L-2} .. U_0: 2 L - 1 on the longest path, and the final store) adds
    H_REL of the value rounded plus H_ABS; the fp32 arithmetic in between adds F_REL of the magnitudes it combined."""
    with np.errstate(invalid="ignore"):  # (signalling NaNs among the inputs)
        i = PR.floats(color)[..., :3].astype(f64)
    h, w = i.shape[:2]
    s = san64(i)
    val, err = [], []
    for lv in range(levels):
        if lv == 0:
            b = box64(s)
            d = san64(b * exposure - threshold)
            e = F_REL * (b * exposure + threshold)
        else:
            d, e = box64(val[-1]), box64(err[-1])
        v = blur64(d)
        val.append(v)
        err.append(blur64(e) + (H_REL + F_REL) * v + H_ABS)
    u, eu = (val[-1], err[-1]) if levels else (None, None)
    for lv in range(levels - 2, -1, -1):
        lh, lw = val[lv].shape[:2]
        t = val[lv] + up64(u, lw, lh)
        eu = err[lv] + up64(eu, lw, lh) + (H_REL + F_REL) * t + H_ABS
        u = np.minimum(t, 65504.0)
    bloom, eb = (up64(u, w, h), up64(eu, w, h)) if levels else (np.zeros_like(i), np.zeros_like(i))
    with np.errstate(invalid="ignore"):
        raw = intensity * bloom + exposure * i
    hh = san64(np.where(np.isnan(raw), 0.0, raw))
    eh = intensity * eb + F_REL * (intensity * bloom + exposure * np.where(np.isfinite(i), np.abs(i), 0.0))
    low = np.maximum(hh - eh, 0.0)  # the operators' slopes, taken at the low end of h's interval where they fall with h
    if op == PR.CLAMP:
        o, slope = np.minimum(hh, 1.0), np.where(low < 1.0, 1.0, 0.0)
    elif op == PR.REINHARD:
        o, slope = hh / (1 + hh), 1.0 / (1 + low) ** 2  # the derivative, which falls with h
    else:
        o = np.minimum(hh * (2.51 * hh + 0.03) / (hh * (2.43 * hh + 0.59) + 0.14), 1.0)
        # the rational's derivative peaks at 1.80 near h = 0.12; it reaches 1 at h = 7.24 (0.08 h^2 - 0.56 h - 0.14 = 0) and is clamped from there
        slope = np.where(low < 7.25, 2.0, 0.0)
    return o, slope * eh + (H_REL + F_REL) * o + H_ABS


@pytest.mark.parametrize("op", [PR.CLAMP, PR.REINHARD, PR.ACES])
@pytest.mark.parametrize("levels", [0, 1, 5])
def test_against_float64(op, levels):
    w, h = 70, 45
    color = PR.random_hdr(w, h, seed=11 + levels, top=0.5, bright=20.0)
    rgb = color[..., :3]
    rgb[(rgb == 0x7bff) | (rgb == 0x7c00)] = 0x4900  # 65504 and +inf become 10: dim enough that most outputs stay below 1
    exposure, threshold, intensity = 0.6, 0.9, 0.05
    ref = PR.run_ref(color, exposure, threshold, intensity, levels, op)
    want, allow = post64(color, exposure, threshold, intensity, levels, op)
    got = PR.floats(ref["color"])[..., :3].astype(f64)
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    over = np.abs(got - want) - allow
    print(f"levels {levels} op {op}: largest error {np.abs(got - want).max():.3e}, largest allowance {allow.max():.3e}, "
          f"smallest margin {-over.max():.3e}")
    assert (over <= 0).all(), f"{int((over > 0).sum())} values outside the allowance, worst by {over.max():.3e}"
    # the allowance is what 2 L roundings can do to a value of at most 1 and to the bloom under it, not a loose net
    assert np.median(allow) < (2 * levels + 2) * H_REL and ((want > 0.02) & (want < 0.98)).mean() > 0.25
    assert np.array_equal(ref["color"][..., 3], color[..., 3])


# ---------------------------------------------------------------- wrong variants are told apart
@pytest.mark.parametrize("variant", sorted(PR.WRONG_VARIANTS))
def test_wrong_variants_are_caught(variant):
    size = (256, 256) if variant == 6 else (42, 30)  # (6 differs by fp32 roundings only: it needs values to show in a half)
    color = PR.random_hdr(*size, seed=21)
    kw = dict(exposure=0.6, threshold=0.9, intensity=0.35, levels=2, tonemap=PR.REINHARD)
    good, bad = PR.run_ref(color, **kw), PR.run_ref(color, variant=variant, **kw)
    differ = (good["color"] != bad["color"]).any(axis=-1)
    assert differ.any(), PR.WRONG_VARIANTS[variant]
    assert np.array_equal(good["color"][..., 3], bad["color"][..., 3])
