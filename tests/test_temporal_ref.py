"""tests/native/temporal_ref.cpp, the scalar restatement of the temporal pass's contract (DESIGN C27-C31), on the CPU:
closed forms on a 64 x 64 image (2 / W is exact there and the identity reproject samples the history texel itself), an
independent float64 implementation within a bound derived from the rounding steps, and six deliberately wrong variants
that must each be told apart."""
import numpy as np
import pytest

import __graft_entry__ as g
import post_ref as PR
import temporal_ref as TR

pkg = g.load_package()
GL = pkg.glmath
f32 = np.float32
N = 64
Z = np.full((N, N), 0.5, f32)
ID = TR.identity()
QUARTER = 0.25  # a power of two: blend * (c - h) is exact, so fma(blend, c - h, h) is one float32 add of exact operands


def plain(seed, n=N):
    """finite positive halves (san is the identity on them)"""
    return PR.random_hdr(n, n, seed, specials=False)


def rgb(bits):
    return PR.floats(bits)[..., :3]


def blend_quarter(c_bits, h_bits):
    c, h = rgb(c_bits), rgb(h_bits)
    return PR.halves(f32(QUARTER) * (c - h) + h)


def san(v):
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, f32(65504.0)), f32(0)).astype(f32)


def cameras(w, h, dyaw=0.05, dpos=(-0.03, 0.02, 0.02)):
    pos, pitch, yaw = (0.0, 2.0, 0.0), 0.1, 1.5
    prev = GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[2]
    cur = GL.scene_data(GL.camera_view(tuple(np.add(pos, dpos)), pitch, yaw + dyaw), w, h)[2]
    return prev, cur


# ---------------------------------------------------------------- closed forms
def test_recurrence_over_three_frames():
    frames = [plain(s) for s in (1, 2, 3)]
    out = TR.run_ref(frames[0], Z, None, ID, QUARTER, TR.NO_CLAMP, history_valid=False)
    assert np.array_equal(out["color"][..., :3], frames[0][..., :3]) and not out["valid"].any()
    assert np.array_equal(out["history"][..., :3], frames[0][..., :3])
    for f in frames[1:]:
        nxt = TR.run_ref(f, Z, out["history"], ID, QUARTER, TR.NO_CLAMP)
        want = blend_quarter(f, out["history"])  # h16(fma(blend, c - h, h))
        assert nxt["valid"].all()
        assert np.array_equal(nxt["color"][..., :3], want)
        assert np.array_equal(nxt["history"][..., :3], want) and not nxt["history"][..., 3].any()
        assert np.array_equal(nxt["color"][..., 3], f[..., 3]), "the alpha half is the frame's"
        out = nxt


def test_constant_image_is_a_fixed_point():
    color = np.empty((N, N, 4), np.uint16)
    color[...] = PR.halves([3.0, 0.7, 12.5, 0.625])
    for flags in (0, TR.NO_CLAMP):
        out = TR.run_ref(color, Z, color, ID, 0.1, flags)
        assert out["valid"].all() and np.array_equal(out["color"], color)


@pytest.mark.parametrize("case", ["blend_1", "invalid", "reset"])
def test_current_colour_alone(case):
    color, hist = PR.random_hdr(N, N, 5), plain(6)
    kw = {"blend_1": dict(blend=1.0), "invalid": dict(blend=0.3, history_valid=False), "reset": dict(blend=0.3, flags=TR.RESET)}[case]
    out = TR.run_ref(color, Z, hist, ID, **kw)
    want = PR.halves(san(rgb(color)))  # san's values are halves already
    assert np.array_equal(out["color"][..., :3], want) and np.array_equal(out["history"][..., :3], want)
    assert np.array_equal(out["color"][..., 3], color[..., 3])
    assert out["valid"].all() == (case == "blend_1")


def test_whole_pixel_translation_shifts_the_history():
    color, hist = plain(7), plain(8)
    out = TR.run_ref(color, Z, hist, TR.ndc_translation(3, -2, N, N), QUARTER, TR.NO_CLAMP)
    valid = np.zeros((N, N), bool)
    valid[2:, :N - 3] = True  # hx = px + 3.5 < 64 and hy = py - 1.5 >= 0
    assert np.array_equal(out["valid"], valid)
    shifted = np.zeros_like(hist)
    shifted[2:, :N - 3] = hist[:N - 2, 3:]
    want = np.where(valid[..., None], blend_quarter(color, shifted), color[..., :3])
    assert np.array_equal(out["color"][..., :3], want)


def neighbourhood(c):
    p = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    stack = np.stack([p[dy:dy + c.shape[0], dx:dx + c.shape[1]] for dy in range(3) for dx in range(3)])
    return stack.min(0), stack.max(0)


def test_history_outliers_are_clamped():
    color = plain(9)
    mn, mx = neighbourhood(rgb(color))
    for value, edge in ((60000.0, mx), (0.0, mn)):
        hist = np.empty_like(color)
        hist[...] = PR.halves(value)
        out = TR.run_ref(color, Z, hist, ID, QUARTER)
        assert np.array_equal(out["color"][..., :3], PR.halves(f32(QUARTER) * (rgb(color) - edge) + edge))
        free = TR.run_ref(color, Z, hist, ID, QUARTER, TR.NO_CLAMP)
        assert np.array_equal(free["color"][..., :3], blend_quarter(color, hist)), "the outlier survives under NO_CLAMP"
        assert not np.array_equal(free["color"], out["color"])


@pytest.mark.parametrize("case", ["w_zero", "w_negative", "nan_x", "nan_w"])
def test_unusable_reprojections_take_the_current_colour(case):
    color, hist = plain(10), plain(11)
    m = TR.identity()
    if case == "w_zero":
        m[3][3] = 0.0
    elif case == "w_negative":
        m[3][3] = -1.0
    elif case == "nan_x":
        m[3][0] = np.nan
    else:
        m[3][3] = np.nan
    out = TR.run_ref(color, Z, hist, m, 0.3)
    assert not out["valid"].any() and np.array_equal(out["color"], color)


# ---------------------------------------------------------------- an independent float64 implementation
def resolve64(color, depth, history, reproject, blend, flags=0, scissor=None):
    """float64 throughout, vectorised, taps by padding and fancy indexing -> (o [sh,sw,3], valid [sh,sw], bound [sh,sw,3]).
    bound: what the fp32 contract may differ by (derivation in test_float64_agrees_on_random_inputs)"""
    H, W = depth.shape
    sx, sy, sw, sh = scissor or (0, 0, W, H)
    c = san(rgb(color)).astype(np.float64)[sy:sy + sh, sx:sx + sw]
    zs = depth.astype(np.float64)[sy:sy + sh, sx:sx + sw]
    hs = rgb(history).astype(np.float64)[sy:sy + sh, sx:sx + sw]
    mn, mx = neighbourhood(c)
    zp = np.pad(zs, 1, mode="edge")
    z = np.stack([zp[dy:dy + sh, dx:dx + sw] for dy in range(3) for dx in range(3)]).max(0)
    M = np.asarray(reproject, np.float64).T  # [row][col]
    px, py = np.meshgrid(np.arange(sx, sx + sw) + 0.5, np.arange(sy, sy + sh) + 0.5)
    v = np.stack([px * 2.0 / W - 1.0, py * 2.0 / H - 1.0, z, np.ones_like(z)], -1)
    q = v @ M.T
    mag = np.abs(v) @ np.abs(M).T  # the sum of the magnitudes of each chain's terms
    with np.errstate(divide="ignore", invalid="ignore"):
        hx, hy = q[..., 0] / q[..., 3] * (W / 2) + W / 2, q[..., 1] / q[..., 3] * (H / 2) + H / 2
        valid = (q[..., 3] > 0) & (hx >= sx) & (hx < sx + sw) & (hy >= sy) & (hy < sy + sh)
        u = 2.0 ** -24
        e_q = 6 * u * mag  # xn or yn (2 roundings, carried through) and the chain's 4
        e_x = (W / 2) * (e_q[..., 0] + np.abs(q[..., 0] / q[..., 3]) * e_q[..., 3]) / q[..., 3] + 6 * u * (np.abs(hx) + W)
        e_y = (H / 2) * (e_q[..., 1] + np.abs(q[..., 1] / q[..., 3]) * e_q[..., 3]) / q[..., 3] + 6 * u * (np.abs(hy) + H)
    hx, hy = np.where(valid, hx, sx + 0.5) - sx, np.where(valid, hy, sy + 0.5) - sy
    fx, fy = hx - 0.5, hy - 0.5
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]
    cx = lambda a: np.clip(a, 0, sw - 1)
    cy = lambda a: np.clip(a, 0, sh - 1)
    top = hs[cy(y0), cx(x0)] * (1 - tx) + hs[cy(y0), cx(x0 + 1)] * tx
    bot = hs[cy(y0 + 1), cx(x0)] * (1 - tx) + hs[cy(y0 + 1), cx(x0 + 1)] * tx
    hist = top * (1 - ty) + bot * ty
    around = np.stack([hs[cy(y0 + j), cx(x0 + i)] for j in range(-1, 3) for i in range(-1, 3)])
    slope = around.max(0) - around.min(0)  # the bilinear surface changes by at most this per texel, this cell and its neighbours
    hc = hist if flags & TR.NO_CLAMP else np.clip(hist, mn, mx)
    use = valid[..., None] & (blend < 1)
    o = np.where(use, hc + np.float64(f32(blend)) * (c - hc), c)
    top_v = np.maximum(around.max(0), c)
    bound = np.where(use, slope * (e_x + e_y)[..., None] + 10 * u * top_v, 0.0) + 2.0 ** -11 * np.abs(o) + 2.0 ** -25
    return o, valid, bound


def compare64(color, depth, history, reproject, blend, flags=0, scissor=None, variant=0):
    H, W = depth.shape
    sx, sy, sw, sh = scissor or (0, 0, W, H)
    out = TR.run_ref(color, depth, history, reproject, blend, flags, scissor=scissor, variant=variant)
    got = rgb(out["color"][sy:sy + sh, sx:sx + sw]).astype(np.float64)
    o, valid, bound = resolve64(color, depth, history, reproject, blend, flags, scissor)
    flipped = valid != out["valid"][sy:sy + sh, sx:sx + sw]
    bad = (np.abs(got - o) > bound).any(-1) & ~flipped
    return bad.mean(), flipped.mean(), valid.mean()


RANDOM = dict(w=96, h=72, scissor=(5, 3, 83, 64))


def random_case(seed=21, w=RANDOM["w"], h=RANDOM["h"]):
    prev, cur = cameras(w, h)
    return PR.random_hdr(w, h, seed), TR.random_depth(w, h, seed + 1), plain(seed + 2, max(w, h))[:h, :w], GL.temporal_reproject(prev, cur)


@pytest.mark.parametrize("flags", [0, TR.NO_CLAMP])
@pytest.mark.parametrize("scissor", [None, RANDOM["scissor"]], ids=["whole", "scissor"])
def test_float64_agrees_on_random_inputs(flags, scissor):
    """The bound, per pixel and channel.  u = 2^-24.  A C0 chain of four terms carries at most 4 roundings of partial sums no
    larger than the sum S of the terms' magnitudes, and its inputs xn, yn two more: |dq| <= 6 u S.  hx = (qx / qw) W/2 + W/2
    moves by (W/2) (|dqx| + |qx/qw| |dqw|) / qw plus the rounding of the reciprocal, the product, the fma and the
    subtraction of 0.5, each at most u (|hx| + W): 6 of them with slack.  The bilinear surface is continuous and changes by at most
    `slope` (the range of the 4 x 4 texels around the sample) per texel, so the sample moves by slope (|dhx| + |dhy|); the
    three lerps, the difference and the fma add at most 10 u times the largest value involved.  The clamp and the blend
    are 1-Lipschitz.  The store rounds to a half: 2^-11 relative, 2^-25 absolute among subnormals."""
    color, depth, hist, m = random_case()
    bad, flipped, valid = compare64(color, depth, hist, m, 0.3, flags, scissor)
    assert 0.1 < valid < 0.9, valid
    assert flipped <= 0.005, flipped
    assert bad == 0.0, bad


def test_cleared_depth_reprojects_under_a_pure_rotation():
    """depth 0 is a point at infinity: q = reproject * (xn, yn, 0, 1) is a direction, rotated like any other"""
    w, h = 96, 72
    prev, cur = cameras(w, h, dyaw=0.08, dpos=(0.0, 0.0, 0.0))
    color, hist = plain(31, 96)[:h, :w], plain(32, 96)[:h, :w]
    bad, flipped, valid = compare64(color, np.zeros((h, w), f32), hist, GL.temporal_reproject(prev, cur), 0.3)
    assert valid > 0.7 and flipped <= 0.005 and bad == 0.0, (valid, flipped, bad)
    # and the shift is the rotation's: about dyaw / fovx of the width, the same at every depth
    m = np.asarray(GL.temporal_reproject(prev, cur), np.float64).T
    q = m @ np.array([0.0, 0.0, 0.0, 1.0])
    assert abs(abs(q[0] / q[3]) * w / 2 - np.tan(0.08) / (np.tan(np.radians(35.0)) * w / h) * w / 2) < 0.05


# ---------------------------------------------------------------- wrong variants
@pytest.mark.parametrize("variant", sorted(TR.WRONG_VARIANTS))
def test_wrong_variants_are_told_apart(variant):
    # variants 5 and 6 differ from the contract by one fp32 rounding: the clamp would hide most of it, and a half keeps it
    # only where the fp32 value sits next to a rounding boundary (about one channel in 2^13), so they get a larger image,
    # no clamp, and every single pixel counts
    subtle = variant in (5, 6)
    color, depth, hist, m = random_case(w=256, h=256) if subtle else random_case()
    blend = 1.0 if variant == 5 else (0.05 if subtle else 0.3)
    kw = dict(flags=TR.NO_CLAMP) if subtle else dict(scissor=RANDOM["scissor"])
    right = TR.run_ref(color, depth, hist, m, blend, **kw)
    wrong = TR.run_ref(color, depth, hist, m, blend, variant=variant, **kw)
    differ = np.any(right["color"] != wrong["color"], axis=-1)
    print(f"variant {variant}: {int(differ.sum())} of {differ.size} pixels differ")
    assert differ.sum() >= (3 if subtle else 0.002 * differ.size), f"variant {variant} ({TR.WRONG_VARIANTS[variant]})"
    if not subtle:  # (one fp32 rounding is inside any float64 bound)
        bad, flipped, _ = compare64(color, depth, hist, m, blend, variant=variant, **kw)
        assert bad + flipped > 0.002, f"variant {variant} passes the float64 check"
