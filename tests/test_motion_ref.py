"""The camera motion blur pass's scalar restatement (tests/native/motion_ref.cpp, DESIGN C67-C72) on the CPU: the velocity
against an fp64 evaluation, the cells against exact integers, the gather against an fp64 statement written from
include/svr_motion.h's definitions (motion_ref.motion64), the numbered wrong variants, and the consequences C72 states.

The allowance of the velocity (u = 2^-24), to first order, from C67's operation count.  xn and yn carry the quotient 2 /
extent and one fma: 2 u (|p + 0.5| 2 / extent + 1).  A row of q is a product and three fmas, each within u of a partial sum
no larger than the sum T of its terms' sizes: 4 u T, beside what xn and yn bring through their columns.  n = q.x (1 / q.w)
takes both rows' errors over |q.w| and two roundings; h = fma(n, half, half) one, of at most |n| half + half; the
difference (p + 0.5) - h one; the product with hs one (hs = 0.5 shutter is exact).  Where l > max_blur: l's three roundings,
the quotient's and the product's are 4 u max_blur, beside the components' own errors and the direction's.  The store rounds
to a half: 2^-11 of the value, or 2^-25 among the subnormals.

The allowance of the gather.  Velocities are halves and depths are compared as they are, so the keys, their maxima, G, n,
rint of the exact products g s, the depth comparison and the zero-offset skip are the same in fp32 and in fp64: no pixel
is left out.  Per tap: e is one fma over an exact product, times rgl, which is a root and a reciprocal: 4 u e; D is one root
of an exact integer: u D; e - D rounds once (at most u (e + D)) and the + 1 once more (at most u: the sum that matters lies
in [0, 1]); sat does not widen an error:
  dw_k = u (5 e_k + 2 D_k + 1).
The sums: acc takes dw_k I_k per tap and one rounding per fma, each at most u times the final sum A = sum w_k I_k +
(n - S) I_p (no term is negative); S likewise, and n - S rounds once more, at most u n; the scaling by 1 / n is exact and
san does not widen an error:
  d_out = (sum dw_k I_k + (sum dw_k + m u S + u n) I_p + (m + 1) u A) / n,   m the taps with an offset,
computed per pixel and channel by motion64 beside the value.  The store rounds the fp32 result to a half.  Nothing here was
tuned; the largest ratio of error to allowance is printed per case."""
import numpy as np
import pytest

import motion_ref as MR

f32 = np.float32
U = MR.U
W, H = 48, 32
CAM = MR.Camera(W, H)

# name -> (this frame's camera position, yaw, view distances, shutter, max_blur, the tap counts the fp64 statement must show)
CASES = {
    "yaw_fast": ((0.0, 0.0, 0.0), 0.45, MR.rolling_dist(W, H, 4), 1.0, 16.0, {16, 32}),
    "strafe_fast": ((3.0, 0.6, 0.0), 0.0, MR.rolling_dist(W, H, 4), 1.0, 16.0, {32}),
    "strafe_clamped": ((3.0, 0.6, 0.0), 0.0, MR.rolling_dist(W, H, 4), 1.0, 4.3, {16}),
    "dolly_long_shutter": ((0.0, 0.0, -1.5), 0.0, MR.rolling_dist(W, H, 4), 4.0, 16.0, None),
    "wall_fast": ((2.0, 0.0, 0.0), 0.0, MR.plane_over_wall(W, H, 24, 2.0, 200.0), 1.0, 16.0, None),
}


@pytest.fixture(scope="module")
def runs():
    """every case's restatement run and fp64 statements, computed once"""
    out = {}
    for name, (pos, yaw, dist, shutter, mb, _) in CASES.items():
        color = MR.random_hdr(W, H, 3, specials=True)
        depth = CAM.depth_of(dist)
        rp = MR.camera_reproject(W, H, pos, yaw)
        r = MR.run_ref(color, depth, rp, shutter, mb)
        out[name] = dict(color=color, depth=depth, reproject=rp, ref=r, m=MR.motion64(r["rgb"], r["v"], r["z"], mb),
                         v=MR.velocity64(depth, rp, shutter, mb, W, H))
    return out


def allowance(m, got32):
    return m["bound"] + 2.0 ** -11 * (np.abs(got32) + m["bound"]) + 2.0 ** -25


# ---------------------------------------------------------------- C67-C69
@pytest.mark.parametrize("name", list(CASES))
def test_velocity_against_fp64(runs, name):
    run = runs[name]
    v64 = run["v"]
    assert (v64["qw"] > 0.05).all(), "the cases keep q.w well away from 0"
    got = MR.floats(run["ref"]["v"]).astype(np.float64)
    tol = v64["bound"] * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(v64["v"]) + 2.0 ** -25
    ratio = (np.abs(got - v64["v"]) / tol).max()
    print(f"{name}: largest velocity error / allowance {ratio:.3f}; longest streak {np.hypot(got[..., 0], got[..., 1]).max():.2f} px")
    assert ratio <= 1.0
    mb = CASES[name][4]
    assert np.abs(got).max() <= np.ceil(mb) and np.hypot(got[..., 0], got[..., 1]).max() > min(mb, 8.0) * 0.9


@pytest.mark.parametrize("name", list(CASES))
def test_prepared_image_and_cells(runs, name):
    """C68's RGB halves are san as a bit operation and the depth's bits travel unchanged; M and G are maxima of keys formed
    through exact integers"""
    run = runs[name]
    assert np.array_equal(run["ref"]["rgb"], MR.san_bits(run["color"][..., :3]))
    assert (run["color"][..., :3] != run["ref"]["rgb"]).any(), "the input holds halves san changes"
    assert np.array_equal(run["ref"]["z"].view(np.uint32), run["depth"].view(np.uint32))
    assert np.array_equal(run["ref"]["M"], run["m"]["M"]) and np.array_equal(run["ref"]["G"], run["m"]["G"])


def test_dead_velocities_and_both_sides_of_the_clamp():
    """q.w <= 0 and non-finite products give velocity 0; a streak longer than max_blur is scaled onto it, a shorter one kept"""
    w = h = 8
    color = MR.random_hdr(w, h, 1)
    depth = np.full((h, w), 0.5, f32)
    depth[0, :4] = [np.nan, np.inf, -np.inf, 1.0]
    rp = MR.affine_reproject(ax=0.5)
    rp[2][3], rp[3][3] = f32(-1.0), f32(0.75)  # q.w = 0.75 - z: 0.25 at 0.5, -0.25 at 1
    v = MR.floats(MR.run_ref(color, depth, rp, 1.0, 16.0)["v"])
    assert (v[0, :4] == 0).all(), "NaN, +-inf (a non-finite product or q.w <= 0) and q.w < 0"
    assert (v[1:, :, 0] != 0).all()
    rp = MR.affine_reproject(ax=0.5, ay=0.5)  # z = 1: (-1, -1) px at shutter 1 in 8 x 8, l = 1.41; z = 0.25: (-0.25, -0.25)
    depth = np.full((h, w), 1.0, f32)
    depth[:, 4:] = 0.25
    v = MR.floats(MR.run_ref(color, depth, rp, 1.0, 1.0)["v"])
    assert (v[:, 4:] == -0.25).all()
    assert (v[:, :4, 0] == v[:, :4, 1]).all() and np.allclose(np.hypot(v[:, :4, 0], v[:, :4, 1]), 1.0, atol=2.0 ** -10) and (v[:, :4] < 0).all()
    huge = MR.affine_reproject(ax=2.0 ** 126)
    v = MR.floats(MR.run_ref(color, np.full((h, w), 2.0 ** 60, f32), huge, 1.0, 16.0)["v"])
    assert (v == 0).all(), "an overflowing product: the velocity is not finite"


def test_no_offset_exceeds_ceil_max_blur_and_neighbours_are_a_pixel_apart():
    """C70's bound over every half up to 16 and both tap tables: |rint(g s)| <= ceil(|g|), which sizes the LDS rim.
    Neighbouring taps of one side lie at most one pixel apart in either count (2 |g| / n <= 1: n is 32 above |g| = 8), so
    their rounded offsets differ by at most one, except between two ties (8 s_j at n = 16: 0.5, 1.5, ... go to 0, 2, 2, 4)"""
    g = np.arange(0, 0x4c01, dtype=np.uint16).view(np.float16).astype(f32)  # 0 .. 16
    assert g[-1] == 16.0
    for n in (16, 32):
        s = ((2 * np.arange(n // 2) + 1) / n).astype(f32)
        prod = g[:, None] * s[None, :]
        assert np.array_equal(prod.astype(np.float64), g[:, None].astype(np.float64) * s[None, :].astype(np.float64)), "the products are exact"
        off = np.rint(prod)
        assert (off <= np.ceil(g)[:, None]).all()
        assert np.array_equal(np.rint(-prod), -off), "the two sides mirror each other"
        use = g <= (8.0 if n == 16 else 16.0)  # L2 > 64 takes 32 taps
        assert (np.diff(prod[use], axis=1) <= 1).all()
        step = np.diff(off[use], axis=1)
        tie = np.abs(prod[use] - np.floor(prod[use])) == 0.5
        assert (step >= 0).all() and (step <= 2).all() and (step[~(tie[:, 1:] & tie[:, :-1])] <= 1).all()


# ---------------------------------------------------------------- C70-C72 against the fp64 statement
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_fp64_statement(runs, name):
    run = runs[name]
    m = run["m"]
    got = MR.floats(run["ref"]["color"][..., :3]).astype(np.float64)
    ratio = (np.abs(got - m["out"]) / allowance(m, got)).max()  # every pixel
    changed = (run["ref"]["color"][..., :3] != run["ref"]["rgb"]).any(-1).mean()
    counts = set(np.unique(m["n"]).tolist())
    print(f"{name}: largest error / allowance {ratio:.3f}; {changed:.2f} of the pixels change; tap counts {sorted(counts)}")
    assert ratio <= 1.0
    assert changed > 0.3
    want = CASES[name][5]
    assert want is None or counts == want
    assert np.array_equal(run["ref"]["color"][..., 3], run["color"][..., 3]), "alpha is copied"
    assert (run["ref"]["S"] <= m["n"]).all() and (m["S"] <= m["n"]).all(), "S <= n"


@pytest.mark.parametrize("variant", list(MR.WRONG_VARIANTS), ids=lambda v: f"{v}_{MR.WRONG_VARIANTS[v].replace(' ', '_').replace('|', '')}")
def test_variants_are_told_apart(runs, variant):
    """each wrong variant leaves an fp64 statement's allowance on at least one case, on a pixel that is compared (every pixel
    is).  7 and 8 change the velocity, so they are held to the velocity's statement; the others to the gather's, which
    starts from the contract's prepared image"""
    caught = []
    for name, (pos, yaw, dist, shutter, mb, _) in CASES.items():
        run = runs[name]
        bad = MR.run_ref(run["color"], run["depth"], run["reproject"], shutter, mb, variant=variant)
        if variant in (7, 8):
            v64 = run["v"]
            tol = v64["bound"] * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(v64["v"]) + 2.0 ** -25
            over = np.abs(MR.floats(bad["v"]).astype(np.float64) - v64["v"]) > tol
        else:
            got = MR.floats(bad["color"][..., :3]).astype(np.float64)
            over = np.abs(got - run["m"]["out"]) > allowance(run["m"], got)
        if over.any():
            caught.append(name)
    print(f"variant {variant} ({MR.WRONG_VARIANTS[variant]}): told apart on {caught}")
    assert caught


# ---------------------------------------------------------------- the consequences
PW, PH = 64, 32  # power-of-two extents: with affine_reproject every product of C67 is exact


def test_identity_leaves_san_of_the_input():
    color = MR.random_hdr(PW, PH, 9, specials=True)
    depth = MR.Camera(PW, PH).depth_of(MR.rolling_dist(PW, PH, 4))
    r = MR.run_ref(color, depth, MR.affine_reproject(), 1.0, 16.0)
    assert (r["v"] == 0).all()
    assert np.array_equal(r["color"][..., :3], MR.san_bits(color[..., :3])) and np.array_equal(r["color"][..., 3], color[..., 3])


def test_closed_shutter_changes_nothing():
    color = MR.random_hdr(W, H, 12, specials=True)
    depth = CAM.depth_of(MR.rolling_dist(W, H, 4))
    rp = MR.camera_reproject(W, H, (3.0, 0.6, 0.0))
    for shutter, mb in ((0.0, 16.0), (1.0, 0.0)):
        assert np.array_equal(MR.run_ref(color, depth, rp, shutter, mb)["color"], color)


def test_a_static_front_plane_over_a_moving_wall_keeps_its_bits():
    """q.x = xn + 0.5 z - 0.5: the plane (z = 1, left of column 24) is still, the wall (z = 0) moves 8 px either way"""
    color = MR.random_hdr(PW, PH, 10, specials=True)
    depth = np.where(np.arange(PW)[None, :] < 24, 1.0, 0.0).astype(f32) * np.ones((PH, 1), f32)
    r = MR.run_ref(color, depth, MR.affine_reproject(ax=0.5, bx=-0.5), 1.0, 16.0)
    v = MR.floats(r["v"])
    assert (v[:, :24] == 0).all() and (v[:, 24:, 0] == 8).all() and (v[..., 1] == 0).all()
    assert np.array_equal(r["color"][:, :24, :3], MR.san_bits(color[:, :24, :3])), "the still plane keeps its bits"
    assert (r["color"][:, 24:, :3] != MR.san_bits(color[:, 24:, :3])).any(-1).mean() > 0.9, "the wall streaks"


def test_a_moving_front_plane_bleeds_over_a_static_wall():
    """q.x = xn + 0.5 z: the plane (z = 1, left of column 24) moves 8 px either way, the wall (z = 0) is still: wall pixels
    beyond the reach (8 px and the cells' +-Rc = 2 cells give G, but a tap's weight needs D < e + 1 = 9) keep their bits,
    pixels next to the edge change"""
    color = MR.random_hdr(PW, PH, 11, specials=True)
    depth = np.where(np.arange(PW)[None, :] < 24, 1.0, 0.0).astype(f32) * np.ones((PH, 1), f32)
    r = MR.run_ref(color, depth, MR.affine_reproject(ax=0.5), 1.0, 16.0)
    v = MR.floats(r["v"])
    assert (v[:, :24, 0] == -8).all() and (v[:, 24:] == 0).all()
    assert np.array_equal(r["color"][:, 24 + 9:, :3], MR.san_bits(color[:, 24 + 9:, :3])), "wall pixels beyond the reach keep their bits"
    assert (r["color"][:, 24:26, :3] != MR.san_bits(color[:, 24:26, :3])).any(-1).mean() > 0.9, "the plane bleeds over the wall"


def test_the_coverage_ramp_is_linear():
    """uniform colours, the moving plane 1.0 and the still wall 0.0: the plane's coverage falls from 1 to 0 across +-e = 8 px
    around the edge and is 0.5 at it.  With 16 taps at 0.5, 1.5, .. 7.5 px either side a pixel d px right of the edge
    (its centre d + 0.5 from it) sees the taps beyond d px to its left: the share (8 - d) / 16 for d = 0 .. 8, every
    weight being exactly 0 or 1 but the last, so the allowance is the store's rounding alone"""
    color = np.zeros((PH, PW, 4), np.uint16)
    color[:, :24, :3] = 0x3c00
    depth = np.where(np.arange(PW)[None, :] < 24, 1.0, 0.0).astype(f32) * np.ones((PH, 1), f32)
    r = MR.run_ref(color, depth, MR.affine_reproject(ax=0.5), 1.0, 16.0)
    row = MR.floats(r["color"][PH // 2, :, 0]).astype(np.float64)
    d = np.arange(PW) - 24.0 + 0.5  # a pixel centre's distance from the edge
    want = np.clip(0.5 - d / 16.0, 0.0, 1.0)
    print("coverage across the edge:", np.round(row[14:36], 4).tolist())
    # a tap's offset is rint of an odd multiple of a half: ties to even move it by half a pixel, 1 / 32 of coverage
    assert np.abs(row - want).max() <= 1.0 / 32.0 + 2.0 ** -11
    assert abs(0.5 * (row[23] + row[24]) - 0.5) <= 2.0 ** -11, "a half at the edge"
    assert (np.diff(row[12:40]) <= 0).all() and row[:15].min() == 1.0 and row[33:].max() == 0.0


def test_a_uniform_velocity_is_the_mean_of_its_taps():
    """every pixel 8 px to the right per half shutter (z = 1 everywhere, q.x = xn - 0.5 z): e = 8 for every texel, so every
    tap within 8 px has weight 1 and the result is the mean of the 16 taps, taken here independently in numpy.  The two
    taps at +-0.5 px round to the pixel itself (ties to even): they have weight 0 and count in n, so the pixel's own colour
    takes their share, which is what reading it at offset 0 gives the mean"""
    color = MR.random_hdr(PW, PH, 13)
    r = MR.run_ref(color, np.ones((PH, PW), f32), MR.affine_reproject(ax=-0.5), 1.0, 16.0)
    assert (MR.floats(r["v"])[..., 0] == 8).all() and (r["v"][..., 1] == 0).all()
    I = MR.floats(MR.san_bits(color[..., :3])).astype(np.float64)
    s = (2 * np.arange(8) + 1) / 16.0
    offs = np.rint(np.concatenate([8 * s, -8 * s])).astype(int)
    assert np.abs(offs).max() == 8 and (offs == 0).sum() == 2
    x = np.arange(PW)
    mean = sum(I[:, np.clip(x + o, 0, PW - 1)] for o in offs) / 16.0
    got = MR.floats(r["color"][..., :3]).astype(np.float64)
    # 16 fmas and the exact scaling: 17 u of the mean, then the store's half
    assert (np.abs(got - mean) <= 17 * U * mean + 2.0 ** -11 * mean * (1 + 17 * U) + 2.0 ** -25).all()
    assert (r["S"] == 14).all()
