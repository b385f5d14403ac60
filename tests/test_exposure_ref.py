"""tests/native/exposure_ref.cpp, the scalar restatement of auto-exposure's contract (DESIGN C38-C42), checked on the CPU.

Three independent statements stand against it:
  * exact rational arithmetic (fractions.Fraction, one explicit round-to-nearest-even to 24 bits per operation) for the
    luminance, and comparisons against the rational bin edges 2^k (1 + j / 8) for the counter: no bit tricks, no floats;
  * known answers worked out by hand (check_* below);
  * exposure_ref.statement64: np.log2 of the true luminances, an exact sort for the percentile window, 2.0 **.

The allowance between the restatement and statement64, derived, not tuned (octaves, on mean_log2):
  * sub-bin width.  A kept pixel is counted at log2(1 + (j + 1/2) / 8) of its octave, and sorting by bin pairs the ranks
    of both statements monotonically, so the means differ by no more than one pixel can.  The widest sub-bin is j = 0,
    log2(9/8) = 0.16993 octaves wide; the allowance takes half of it, 0.08496.  (A pixel sitting exactly on that bin's
    lower edge is log2(17/16) = 0.08746 from the arithmetic midpoint's logarithm, 0.0025 more: only a plane made of such
    pixels can show it, and those planes are pinned exactly by the known answers, not by this allowance.)
  * fp32 luminance against fp64: three roundings and three rounded weights, below 4 * 2^-24 relative, 3.5e-7 octaves
    (the fp32 weights sum to 1 exactly, the decimal ones to 1 as well: no bias);
    a pixel this moves into a neighbouring bin is still within the sub-bin term of its own logarithm plus this;
  * mean_log2 is rounded to fp32 once: |mean| < 16, half an ulp is 2^-21 = 4.8e-7.
  MEAN_ALLOW = log2(9/8) / 2 + 1e-6.  A pixel within 1e-6 relative of the black threshold 2^-16 could be counted by one
  statement and not by the other; the cases hold none (asserted).
On log2(target), where the clamp does not bind: MEAN_ALLOW, plus the polynomial's error, measured here against fp64 over a
dense sweep and held below POLY_REL = 2^-23 (measured: 6.33e-8), plus two fp32 roundings (key * 2^x and 2^x's last fma
are in the sweep): TARGET_ALLOW = MEAN_ALLOW + log2(1 + POLY_REL) + 2 * 2^-24 * log2(e)."""
from fractions import Fraction

import numpy as np
import pytest

import exposure_ref as ER

f32 = np.float32
MEAN_ALLOW = 0.5 * np.log2(9 / 8) + 1e-6
POLY_REL = 2.0 ** -23
TARGET_ALLOW = MEAN_ALLOW + np.log2(1 + POLY_REL) + 2 * 2.0 ** -24 * np.log2(np.e)


# ---------------------------------------------------------------- exact arithmetic
def rnd32(q):
    """a positive rational rounded to the nearest fp32 (ties to even), as a Fraction; normal range only"""
    if q == 0:
        return q
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and e > -126
    unit = Fraction(2) ** (e - 23)
    n = q / unit
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2):
        r += 1
    return r * unit


def half_exact(bits):
    """san() of a half's value, as a Fraction"""
    bits = int(bits)
    e, m = (bits >> 10) & 31, bits & 0x3ff
    if bits & 0x8000 or (e == 31 and m):
        return Fraction(0)  # negatives, -0 and NaN
    if e == 31:
        return Fraction(65504)
    return Fraction(m, 1 << 24) if e == 0 else Fraction(1024 + m, 1024) * Fraction(2) ** (e - 15)


WEIGHTS = [Fraction(float(f32(w))) for w in (0.2126, 0.7152, 0.0722)]


def lum_exact(texel):
    r, g, b = (half_exact(texel[c]) for c in range(3))
    return rnd32(WEIGHTS[2] * b + rnd32(WEIGHTS[1] * g + rnd32(WEIGHTS[0] * r)))


def counter_exact(L):
    if L < Fraction(1, 1 << 16):
        return 256
    assert L < 1 << 16
    for k in range(-16, 16):
        if L < Fraction(2) ** (k + 1):
            j = int((L / Fraction(2) ** k - 1) * 8)  # the floor of a rational in [0, 8)
            return 8 * (k + 16) + j
    raise AssertionError


def hist_exact(color, scissor=None):
    h, w = color.shape[:2]
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    out = np.zeros(257, np.uint32)
    for y in range(sy, sy + sh):
        for x in range(sx, sx + sw):
            out[counter_exact(lum_exact(color[y, x]))] += 1
    return out


def rep(counter):
    """log2 of the luminance a bin's pixels are counted at, fp64"""
    return (counter >> 3) - 16 + np.log2(1 + ((counter & 7) + 0.5) / 8)


def grey_counter(value):
    return counter_exact(lum_exact(ER.halves([value] * 3)))


# ---------------------------------------------------------------- the pieces
def test_exp2_polynomial_against_fp64():
    frac = np.linspace(0.0, 1.0, (1 << 21) + 1).astype(f32)
    worst = 0.0
    for n in (-16, -7, -1, 0, 3, 15):
        x = (frac[:-1] + f32(n)).astype(f32)
        got = ER.exp2_poly(x).astype(np.float64)
        worst = max(worst, float(np.abs(got / 2.0 ** x.astype(np.float64) - 1).max()))
    print(f"2^x polynomial: worst relative error {worst:.3e}")
    assert worst < POLY_REL
    ints = np.arange(-16, 17, dtype=f32)
    assert np.array_equal(ER.exp2_poly(ints), (2.0 ** ints.astype(np.float64)).astype(f32))  # exact at integers
    tiny = ER.exp2_poly(np.array([-1e-9, 1e-9, -0.0], f32))  # a fraction that rounds to 1.0 takes the polynomial's top
    assert np.all(np.abs(tiny.astype(np.float64) - 1) < 2 * POLY_REL)


def test_counters_at_every_bin_edge():
    edges = np.array([2.0 ** k * (1 + j / 8) for k in range(-16, 16) for j in range(8)], f32)
    assert np.array_equal(ER.counters(edges), np.arange(256, dtype=np.uint32))
    below = np.nextafter(edges, f32(0))
    assert np.array_equal(ER.counters(below), np.concatenate([[256], np.arange(255)]).astype(np.uint32))
    # the largest luminance three halves can give stays in the last bin; zero and what is below 2^-16 are black
    top = float(lum_exact(ER.halves([65504.0] * 3)))
    assert top < 65536 and ER.counters(np.array([top, 65535.996, 0.0, 2.0 ** -17, 1e-30], f32)).tolist() == [255, 255, 256, 256, 256]


def test_bin_edges_as_halves_against_exact_arithmetic():
    """every bin edge a half can hold, and the half just below it, as grey and as single-channel texels"""
    edges = ER.halves([2.0 ** k * (1 + j / 8) for k in range(-16, 16) for j in range(8) if 2.0 ** k * (1 + j / 8) >= 2.0 ** -24])
    vals = np.unique(np.concatenate([edges, edges - 1]))
    color = np.zeros((4, vals.size, 4), np.uint16)
    color[0, :, :3] = vals[:, None]
    for c in range(3):
        color[1 + c, :, c] = vals
    hist, st = ER.run_ref(color)
    want = hist_exact(color)
    assert np.array_equal(hist, want[:256]) and st["black"] == want[256] and st["counted"] == want[:256].sum()
    assert st["counted"] + st["black"] == color.shape[0] * color.shape[1]


def test_specials_are_black_or_clamped():
    one = 0x3c00
    texels = {"nan": 0x7e00, "-nan": 0xfe00, "snan": 0x7c01, "-inf": 0xfc00, "-1": 0xbc00, "-0": 0x8000, "0": 0, "min denormal": 1, "-min denormal": 0x8001}
    for name, bits in texels.items():
        hist, st = ER.run_ref(ER.grey(1, 1, bits))
        assert st["black"] == 1 and st["counted"] == 0 and not hist.any(), name
        # ... and beside a lit channel it adds nothing
        mixed = np.array([[[bits, one, bits, 0]]], np.uint16)
        assert np.array_equal(ER.run_ref(mixed)[0], ER.run_ref(np.array([[[0, one, 0, 0]]], np.uint16))[0]), name
    for bits in (0x7c00, 0x7bff):  # +inf counts as 65504
        hist, st = ER.run_ref(ER.grey(1, 1, bits))
        assert hist[255] == 1 and st["black"] == 0
    assert np.array_equal(ER.run_ref(ER.grey(1, 1, 0x7c00))[1]["mean_log2"], ER.run_ref(ER.grey(1, 1, 0x7bff))[1]["mean_log2"])


# ---------------------------------------------------------------- known answers; each takes the variant it is run on
def check_one_value(variant=0):
    for value in (1.0, 0.18, 3.0e-4, 65504.0, 2.0 ** -14):
        c = grey_counter(value)
        hist, st = ER.run_ref(ER.grey(5, 7, ER.halves(value)), ER.meter(min_exposure=1e-9, max_exposure=1e9), variant=variant)
        want = np.zeros(256, np.uint32)
        want[c] = 35
        assert np.array_equal(hist, want), value
        assert (st["counted"], st["black"], st["meters"]) == (35, 0, 1)
        assert st["mean_log2"] == f32(rep(c)), value
        true_target = 0.18 * 2.0 ** -float(st["mean_log2"])
        assert st["target"] == st["exposure"] and abs(float(st["target"]) / float(f32(0.18)) * 0.18 / true_target - 1) < POLY_REL + 2.0 ** -23


def check_two_values(variant=0):
    dark, bright = ER.halves(0.25), ER.halves(4.0)
    color = ER.grey(4, 6, dark)
    color[2:] = ER.grey(2, 6, bright)
    rd, rb = rep(grey_counter(0.25)), rep(grey_counter(4.0))
    for low, high, want in ((0.0, 0.5, rd), (0.5, 1.0, rb), (0.0, 1.0, (12 * rd + 12 * rb) / 24), (0.25, 0.75, (6 * rd + 6 * rb) / 24 * 2)):
        _, st = ER.run_ref(color, ER.meter(low_fraction=low, high_fraction=high), variant=variant)
        assert st["mean_log2"] == f32(want), (low, high)
        assert st["counted"] == 24


def check_window_ends(variant=0):
    """T = 10: ceil(0.55 * 10) = 6 keeps the five dark pixels and one bright one; floor(0.35 * 10) = 3 drops three dark ones"""
    color = ER.grey(1, 10, ER.halves(0.25))
    color[0, 5:] = ER.grey(1, 5, ER.halves(4.0))[0]
    rd, rb = rep(grey_counter(0.25)), rep(grey_counter(4.0))
    _, st = ER.run_ref(color, ER.meter(high_fraction=0.55), variant=variant)
    assert st["mean_log2"] == f32((5 * rd + rb) / 6)
    _, st = ER.run_ref(color, ER.meter(low_fraction=0.35, high_fraction=0.5), variant=variant)
    assert st["mean_log2"] == f32(rd)
    _, st = ER.run_ref(color, ER.meter(low_fraction=0.35, high_fraction=0.95), variant=variant)
    assert st["mean_log2"] == f32((2 * rd + 5 * rb) / 7)


def check_black_is_outside_the_window(variant=0):
    """half the plane black, a quarter dark, a quarter bright: the upper half of the NON-black pixels is the bright quarter"""
    color = ER.grey(4, 4, 0)
    color[2] = ER.grey(1, 4, ER.halves(0.25))[0]
    color[3] = ER.grey(1, 4, ER.halves(4.0))[0]
    hist, st = ER.run_ref(color, ER.meter(low_fraction=0.5), variant=variant)
    assert (st["counted"], st["black"]) == (8, 8) and hist.sum() == 8 and hist[0] == 0
    assert st["mean_log2"] == f32(rep(grey_counter(4.0)))


def check_empty_windows(variant=0):
    prev = dict(ER.FIRST_STATE, exposure=f32(3.5), target=f32(2.25), mean_log2=f32(-1.5), counted=99, black=7, meters=4)
    hist, st = ER.run_ref(ER.grey(3, 3, 0), prev=prev, snap=False, variant=variant)  # T == 0
    assert (st["exposure"], st["target"], st["mean_log2"]) == (f32(3.5), f32(2.25), f32(-1.5))
    assert (st["counted"], st["black"], st["meters"]) == (0, 9, 5) and not hist.any()
    # T = 1 with a window that comes out empty: floor(0.5) = 0 .. ceil(0.4) = 1 keeps it; floor(0.5 * 3) = 1 .. ceil(0.3 * 3) = 1 does not
    one = ER.grey(1, 1, 0x3c00)
    assert ER.run_ref(one, ER.meter(low_fraction=0.3, high_fraction=0.4), prev=prev, snap=False, variant=variant)[1]["mean_log2"] != f32(-1.5)
    hist, st = ER.run_ref(ER.grey(1, 3, 0x3c00), ER.meter(low_fraction=0.5, high_fraction=0.3 + 0.2000001), prev=prev, variant=variant)
    assert st["mean_log2"] != f32(-1.5)  # 0.5000001 * 3 rounds up to 2: kept
    hist, st = ER.run_ref(ER.grey(1, 2, 0x3c00), ER.meter(low_fraction=0.5, high_fraction=0.5000001), prev=prev, variant=variant)
    assert st["counted"] == 2 and st["mean_log2"] != f32(-1.5)  # ranks [1, 2)
    hist, st = ER.run_ref(ER.grey(1, 1, 0x3c00), ER.meter(low_fraction=0.999, high_fraction=1.0), prev=prev, snap=True, variant=variant)
    assert st["mean_log2"] != f32(-1.5)  # floor(0.999) = 0
    hist, st = ER.run_ref(ER.grey(1, 4, 0x3c00), ER.meter(low_fraction=0.25, high_fraction=0.25000001), prev=prev, snap=True, variant=variant)
    # f32(0.25000001) == 0.25: the caller's side refuses it (high must exceed low); the arithmetic leaves the state alone
    assert (st["exposure"], st["target"], st["mean_log2"], st["counted"], st["meters"]) == (f32(3.5), f32(2.25), f32(-1.5), 4, 5)


def check_clamp_and_adapt(variant=0):
    """a dark plane wants an exposure far above max_exposure = 4: target = 4 exactly, and from 1.0 at adapt 0.5 the
    exposure is fmaf(0.5, 3, 1) = 2.5 exactly; a bright one against min_exposure = 0.5: fmaf(0.25, -0.5, 1) = 0.875"""
    prev = dict(ER.FIRST_STATE, meters=1)
    _, st = ER.run_ref(ER.grey(2, 2, ER.halves(1e-3)), ER.meter(max_exposure=4.0, adapt=0.5), prev=prev, snap=False, variant=variant)
    assert (st["target"], st["exposure"], st["meters"]) == (f32(4.0), f32(2.5), 2)
    _, st = ER.run_ref(ER.grey(2, 2, ER.halves(900.0)), ER.meter(min_exposure=0.5, adapt=0.25), prev=prev, snap=False, variant=variant)
    assert (st["target"], st["exposure"]) == (f32(0.5), f32(0.875))
    _, st = ER.run_ref(ER.grey(2, 2, ER.halves(900.0)), ER.meter(min_exposure=0.5, adapt=0.0), prev=prev, snap=False, variant=variant)
    assert (st["target"], st["exposure"]) == (f32(0.5), f32(1.0))


def adapted(adapt, target, exposure):
    """fmaf(adapt, target - exposure, exposure) for an adapt that is a power of two: the fp32 difference, then a product
    and a sum that are exact in fp64, rounded once"""
    d = f32(target) - f32(exposure)
    return f32(np.float64(f32(adapt)) * np.float64(d) + np.float64(f32(exposure)))


def check_snap(variant=0):
    prev = dict(ER.FIRST_STATE, exposure=f32(8.0))
    _, st = ER.run_ref(ER.grey(2, 2, ER.halves(0.5)), ER.meter(adapt=0.25), prev=prev, snap=True, variant=variant)
    assert st["exposure"] == st["target"] and st["target"] < 1
    _, st2 = ER.run_ref(ER.grey(2, 2, ER.halves(0.5)), ER.meter(adapt=0.25), prev=prev, snap=False, variant=variant)
    assert st2["exposure"] == adapted(0.25, st2["target"], 8.0)


CHECKS = [check_one_value, check_two_values, check_window_ends, check_black_is_outside_the_window, check_empty_windows, check_clamp_and_adapt,
          check_snap]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_known_answers(check):
    check()


@pytest.mark.parametrize("variant", sorted(ER.WRONG_VARIANTS))
def test_wrong_variants_are_caught(variant):
    caught = []
    for check in CHECKS:
        try:
            check(variant)
        except AssertionError:
            caught.append(check.__name__)
    print(ER.WRONG_VARIANTS[variant], "caught by", caught)
    assert caught, ER.WRONG_VARIANTS[variant]


# ---------------------------------------------------------------- against exact arithmetic and the fp64 statement
CASES = [(37, 23, 5, None, {}), (130, 67, 6, None, {}), (130, 67, 7, (3, 5, 117, 59), dict(low_fraction=0.1, high_fraction=0.9)),
         (64, 48, 8, (1, 0, 63, 47), dict(low_fraction=0.5, high_fraction=0.95, key=0.5))]


@pytest.mark.parametrize("w,h,seed,scissor,kw", CASES)
def test_against_the_fp64_statement(w, h, seed, scissor, kw):
    color = ER.random_hdr(w, h, seed)
    m = ER.meter(**kw)
    hist, st = ER.run_ref(color, m, scissor=scissor)
    lum = ER.luminance64(color, scissor)
    assert not (np.abs(lum / 2.0 ** -16 - 1) < 1e-6).any()
    mean, target, T, kept = ER.statement64(color, m, scissor)
    assert (st["counted"], st["black"]) == (T, lum.size - T) and hist.sum() == T and kept > 100
    err = abs(float(st["mean_log2"]) - mean)
    terr = abs(np.log2(float(st["target"]) / target))
    print(f"mean_log2 {float(st['mean_log2']):+.5f} against {mean:+.5f}: off by {err:.5f} (allowed {MEAN_ALLOW:.5f}); log2 target off by {terr:.5f}")
    assert err <= MEAN_ALLOW and terr <= TARGET_ALLOW
    assert st["exposure"] == st["target"]
    if w * h < 1000:  # the histogram itself, pixel by pixel in exact arithmetic
        want = hist_exact(color, scissor)
        assert np.array_equal(hist, want[:256]) and st["black"] == want[256]


def test_histogram_against_exact_arithmetic_under_a_scissor():
    color = ER.random_hdr(41, 29, 9)
    for scissor in (None, (3, 5, 31, 19), (40, 28, 1, 1), (0, 0, 2, 1), (7, 3, 1, 5)):
        hist, st = ER.run_ref(color, scissor=scissor)
        want = hist_exact(color, scissor)
        assert np.array_equal(hist, want[:256]) and st["black"] == want[256], scissor


def test_a_chain_of_meters():
    planes = [ER.random_hdr(33, 21, s, lo=-6 + 3 * s, hi=2 + 3 * s) for s in range(3)]
    st, m = None, ER.meter(adapt=0.25)
    for i, p in enumerate(planes):
        prev = st
        _, st = ER.run_ref(p, m, prev=prev, snap=i == 0)
        assert st["meters"] == i + 1
        if i == 0:
            assert st["exposure"] == st["target"]
        else:
            assert st["exposure"] == adapted(0.25, st["target"], prev["exposure"])
            assert st["exposure"] != st["target"]
