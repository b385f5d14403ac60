"""The depth of field pass's scalar restatement (tests/native/dof_ref.cpp, DESIGN C61-C66) on the CPU: the prepared image and
the cells against numpy, the gather against an fp64 statement written from include/svr_dof.h's definitions (dof_ref.dof64),
the numbered wrong variants, the consequences C66 states, the tap table from its formula, and the two caller-side helpers.

The allowance of the gather (u = 2^-24), to first order, from the operation counts of C65 and C66.  Radii are halves, so
|c|, the comparison c_k > c_p, the minimum, e^2 (22 bits) and max(e^2, 1) are exact in fp32 and in fp64 alike, and so are
the cell maxima and g.  Per tap: dist is one correctly rounded root of an exact integer (u dist); e - dist rounds once (at
most u (e + dist)) and the + 1 once more (at most u: the sum that matters lies in [0, 1]); sat does not widen an error; the
quotient rounds once:
  dw_k = u (2 dist_k + e_k + 1) / max(e_k^2, 1) + u w_k.
The sums: acc takes dw_k I_k per tap and one rounding per fma, each at most u times the final sum (the terms are not
negative); W likewise.  The quotient rounds once, san does not widen an error:
  d_out = (sum dw_k I_k + n u acc + out (sum dw_k + n u W)) / W + u out,
computed per pixel and channel by dof64 beside the value.  The store rounds the fp32 result to a half: 2^-11 of it, or
2^-25 among the subnormals.  Nothing here was tuned; the largest ratio of error to allowance is printed per case.
The one discrete decision fp32 and fp64 can take differently is rint(u_k g) near a half-integer: a pixel with a tap whose
u_k g lies within 2^-18 of one in fp64 is left out, and at most 1 % of a case's pixels may be (asserted)."""
import math

import numpy as np
import pytest

import __graft_entry__ as g
import dof_ref as DR

GL = g.load_package().glmath
f32 = np.float32
U = DR.U
W, H = 48, 32
CAM = DR.Camera(W, H)
UNIT = DR.UnitCamera()

# name -> (camera, view distances, focus_distance, blur_scale, max_radius)
CASES = {
    "rolling_far": (CAM, DR.rolling_dist(W, H, 4), 4.0, 9.25, 16.0),      # mostly behind the focus; cleared pixels at 9.25
    "rolling_near": (CAM, DR.rolling_dist(W, H, 4), 25.0, 1.5, 16.0),     # mostly in front of it, clamped at -16
    "rolling_clamped": (CAM, DR.rolling_dist(W, H, 4), 8.0, 6.0, 4.3),    # both sides clamped, Rc = 1
    "shallow": (CAM, DR.rolling_dist(W, H, 4), 4.0, 1.2, 16.0),           # g about 1: inner taps fall on the pixel itself
    "plane_over_wall": (CAM, DR.plane_over_wall(W, H, 32, 2.0, 8.0), 8.0, 4.0, 16.0),  # the edge on a tile's border
}


@pytest.fixture(scope="module")
def runs():
    """every case's restatement run and fp64 statement, computed once"""
    out = {}
    for name, (cam, dist, focus, blur, mr) in CASES.items():
        color = DR.random_hdr(W, H, 3, specials=True)
        depth = cam.depth_of(dist)
        r = DR.run_ref(color, depth, cam.terms, focus, blur, mr)
        out[name] = dict(color=color, depth=depth, ref=r, m=DR.dof64(r["prepared"], mr))
    return out


def allowance(m, got32):
    return m["bound"] + 2.0 ** -11 * (np.abs(got32) + m["bound"]) + 2.0 ** -25


# ---------------------------------------------------------------- C61-C63
@pytest.mark.parametrize("name", list(CASES))
def test_prepared_image_and_cells(runs, name):
    """C62's RGB halves are san as a bit operation; c is C61 within its three fp32 roundings (iz, the fma, the product:
    u (blur focus |iz| + 2 |r|)) and the half's; M and g are exact maxima"""
    cam, dist, focus, blur, mr = CASES[name]
    run = runs[name]
    prep = run["ref"]["prepared"]
    assert np.array_equal(prep[..., :3], DR.san_bits(run["color"][..., :3]))
    assert (run["color"][..., :3] != prep[..., :3]).any(), "the input holds halves san changes"
    r64 = DR.radius64(run["depth"], cam.terms, focus, blur, mr)
    iz = np.abs(run["depth"].astype(np.float64) * cam.terms[0] + cam.terms[1])
    tol = U * (blur * focus * iz + 2 * np.abs(r64)) * (1 + 2.0 ** -11) + 2.0 ** -11 * np.abs(r64) + 2.0 ** -25
    c = DR.floats(prep[..., 3]).astype(np.float64)
    assert (np.abs(c - r64) <= tol).all() and np.abs(c).max() <= math.ceil(mr)
    cleared = run["depth"].view(np.uint32) == 0  # no special case: iz = inv_z_bias
    assert cleared.any() == (name != "plane_over_wall") and (c[cleared] == DR.floats(DR.halves(r64[cleared]))).all()
    pad = np.zeros(((H + 7) // 8 * 8, (W + 7) // 8 * 8))
    pad[:H, :W] = np.abs(c)
    assert np.array_equal(run["ref"]["M"], pad.reshape((H + 7) // 8, 8, (W + 7) // 8, 8).max(axis=(1, 3)).astype(f32))
    assert np.array_equal(run["ref"]["g"], run["m"]["g"].astype(f32))


def test_a_nan_radius_counts_as_zero_and_both_sides_clamp():
    color = DR.random_hdr(8, 8, 1)
    depth = UNIT.depth_of(np.full((8, 8), 4.0))
    depth[0, 0], depth[0, 1], depth[0, 2], depth[0, 3] = np.nan, np.inf, -np.inf, 1.0 / 1024
    c = DR.floats(DR.run_ref(color, depth, UNIT.terms, 4.0, 8.0, 5.0)["prepared"][..., 3])
    assert c[0, 0] == 0 and c[0, 1] == -5 and c[0, 2] == 5 and c[0, 3] == 5 and (c[1:] == 0).all()


# ---------------------------------------------------------------- C64-C66 against the fp64 statement
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_fp64_statement(runs, name):
    run = runs[name]
    m = run["m"]
    got = DR.floats(run["ref"]["color"][..., :3]).astype(np.float64)
    share = m["tie"].mean()
    ok = ~m["tie"]
    ratio = (np.abs(got - m["out"]) / allowance(m, got))[ok].max()
    changed = (run["ref"]["color"][..., :3] != run["ref"]["prepared"][..., :3]).any(-1).mean()
    print(f"{name}: {share:.4f} of the pixels left out; largest error / allowance {ratio:.3f}; {changed:.2f} of the pixels change")
    assert share <= 0.01
    assert ratio <= 1.0
    assert changed > 0.3
    assert np.array_equal(run["ref"]["color"][..., 3], run["color"][..., 3]), "alpha is copied"


# ---------------------------------------------------------------- the wrong variants
@pytest.mark.parametrize("variant", list(DR.WRONG_VARIANTS), ids=lambda v: f"{v}_{DR.WRONG_VARIANTS[v].replace(' ', '_').replace('/', 'over')}")
def test_variants_are_told_apart(runs, variant):
    """each wrong variant leaves the fp64 statement's allowance on at least one case, on a pixel that is compared"""
    caught = []
    for name, (cam, dist, focus, blur, mr) in CASES.items():
        run = runs[name]
        bad = DR.floats(DR.run_ref(run["color"], run["depth"], cam.terms, focus, blur, mr, variant=variant)["color"][..., :3]).astype(np.float64)
        with np.errstate(invalid="ignore"):
            over = np.abs(bad - run["m"]["out"]) > allowance(run["m"], bad)
        if over[~run["m"]["tie"]].any():
            caught.append(name)
    print(f"variant {variant} ({DR.WRONG_VARIANTS[variant]}): told apart on {caught}")
    assert caught


# ---------------------------------------------------------------- the consequences C66 states
def test_everything_at_the_focus_distance_leaves_san_of_the_input():
    color = DR.random_hdr(W, H, 9, specials=True)
    for cam, focus in ((UNIT, 4.0), (CAM, 7.3)):
        r = DR.run_ref(color, cam.depth_of(np.full((H, W), focus)), cam.terms, focus, 12.0, 16.0)
        assert np.abs(DR.floats(r["prepared"][..., 3])).max() < 0.5  # exactly 0 under the unit camera, a rounding's worth under the project's
        assert np.array_equal(r["color"][..., :3], DR.san_bits(color[..., :3])) and np.array_equal(r["color"][..., 3], color[..., 3])
    assert (DR.floats(DR.run_ref(color, UNIT.depth_of(np.full((H, W), 4.0)), UNIT.terms, 4.0, 12.0, 16.0)["prepared"][..., 3]) == 0).all()


@pytest.mark.parametrize("max_radius", [4.0, 12.0])
def test_a_sharp_pixel_out_of_reach_keeps_its_bits(max_radius):
    """a near plane (radius -max_radius) left of column 8 over a wall at the focus distance (radius 0 exactly): wall pixels
    farther than R + 8 Rc from the plane leave as san(input); pixels next to the edge change"""
    w, h, edge = 64, 24, 8
    R = math.ceil(max_radius)
    reach = R + 8 * ((R + 7) // 8)
    color = DR.random_hdr(w, h, 10, specials=True)
    r = DR.run_ref(color, UNIT.depth_of(DR.plane_over_wall(w, h, edge, 1.0, 4.0)), UNIT.terms, 4.0, 16.0, max_radius)
    c = DR.floats(r["prepared"][..., 3])
    assert (c[:, :edge] == -max_radius).all() and (c[:, edge:] == 0).all()
    assert np.array_equal(r["color"][:, edge + reach:, :3], DR.san_bits(color[:, edge + reach:, :3]))
    assert (r["color"][:, edge:edge + 2, :3] != DR.san_bits(color[:, edge:edge + 2, :3])).any(-1).mean() > 0.9, "the plane bleeds over the wall"
    # ... and not the reverse: a wall in front of the focus is no wider than the plane behind it is blurred
    r2 = DR.run_ref(color, UNIT.depth_of(DR.plane_over_wall(w, h, edge, 4.0, 1e6)), UNIT.terms, 4.0, 16.0, max_radius)
    assert np.array_equal(r2["color"][:, :edge, :3], DR.san_bits(color[:, :edge, :3])), "a blurred background leaves the sharp plane alone"


def test_one_contributing_tap_is_exact():
    """a lone blurred pixel among sharp ones gathers itself alone with w_0 = 1 / c^2: fma(w_0, I, 0) / w_0 is I after the
    store's rounding, for every finite positive half I and every radius: two fp32 roundings (2 u) cannot move a half (2^-11)"""
    I = np.arange(1, 0x7c00, dtype=np.uint16).view(np.float16).astype(f32)
    for c in np.concatenate([np.linspace(1.0, 16.0, 61), [1.0009765625, 15.9921875, 3.0]]).astype(np.float16).astype(f32):
        w0 = f32(1.0) / (c * c)
        with np.errstate(under="ignore"):
            out = ((w0 * I).astype(f32) / w0).astype(f32).astype(np.float16).astype(f32)
        assert np.array_equal(out, I), float(c)
    # through the restatement: one pixel behind the focus, its neighbours at it
    w, h = 24, 24
    color = DR.random_hdr(w, h, 11, specials=True)
    dist = np.full((h, w), 4.0)
    dist[12, 12] = 16.0
    r = DR.run_ref(color, UNIT.depth_of(dist), UNIT.terms, 4.0, 4.0, 16.0)
    assert DR.floats(r["prepared"][12, 12, 3]) == 3.0 and r["g"].max() == 3.0
    assert np.array_equal(r["color"][..., :3], DR.san_bits(color[..., :3]))


def test_zero_blur_changes_nothing():
    color = DR.random_hdr(W, H, 12, specials=True)
    depth = CAM.depth_of(DR.rolling_dist(W, H, 4))
    for blur, mr in ((0.0, 16.0), (6.0, 0.0)):
        assert np.array_equal(DR.run_ref(color, depth, CAM.terms, 4.0, blur, mr)["color"], color)


# ---------------------------------------------------------------- the tap table
def test_tap_table_is_its_formula():
    t = DR.tap_table()
    assert t.shape == (49, 2) and np.array_equal(t.view(np.uint32), DR.ref_taps())
    # the library's copy (csrc/svr_dof_taps.h) holds the same literals
    import re
    text = open(g.PKG_DIR + "/csrc/svr_dof_taps.h").read()
    lits = re.findall(r"\{(-?0x[0-9a-f.]+p[+-]\d+)f, (-?0x[0-9a-f.]+p[+-]\d+)f\}", text)
    assert len(lits) == 49
    assert np.array_equal(np.array([[float.fromhex(a), float.fromhex(b)] for a, b in lits], np.float64).astype(f32).view(np.uint32), t.view(np.uint32))
    rad = np.hypot(t[:, 0].astype(np.float64), t[:, 1].astype(np.float64))
    assert rad[0] == 0 and np.allclose(rad[1:9], 1 / 3, atol=1e-7) and np.allclose(rad[9:25], 2 / 3, atol=1e-7) and np.allclose(rad[25:], 1.0, atol=1e-7)
    assert (np.abs(t) <= 1).all(), "no offset leaves the window"
    assert t[1, 1] == 0 and t[9, 1] > 0 and t[25, 1] == 0, "only the even ring is turned"


# ---------------------------------------------------------------- the caller's helpers
def test_thin_lens_blur_scale():
    for fl, n, zf, sensor, height in ((0.05, 1.8, 4.0, 0.024, 2160), (0.035, 2.8, 1.5, 0.024, 1080), (0.085, 1.4, 10.0, 0.036, 54)):
        f, N, z, s, h = (float(f32(v)) for v in (fl, n, zf, sensor, height))
        coc_at_infinity = f * f / (N * (z - f))  # the diameter on the sensor: aperture f / N times the magnification f / (z - f)
        want = 0.5 * coc_at_infinity * h / s
        got = GL.dof_blur_scale(fl, n, zf, sensor, height)
        assert got.dtype == f32 and abs(float(got) - want) <= 2.0 ** -24 * want * (1 + 1e-6)


@pytest.mark.parametrize("jitter", [None, (0.37, -0.21)])
def test_depth_terms_recover_the_view_distance(jitter):
    """depth from the project's projection (fp32, glm's order), then 1 / fma(depth, s, b) against the true distance D.  With
    A = proj[2][2], B = proj[3][2]: clip z = A (-D) + B takes a rounding in the product and one in the sum, the division
    by D one more, so depth is off by at most u (A D + 2 |B - A D|) / D; s and b carry one rounding each and the fma one:
    the recovered 1 / D is off, relative to 1 / D, by at most u (2 A D + 3 |B - A D|) / B + u, to first order (the cast of
    the fma's fp64 evaluation here adds none).  A jitter moves the x and y rows only."""
    proj = CAM.proj.copy()
    if jitter:
        proj = GL.jitter_projection(proj, jitter[0], jitter[1], W, H)
    s, b = GL.dof_depth_terms(proj)
    assert s.dtype == f32 and (s, b) == tuple(f32(v) for v in CAM.terms), "a jitter does not move the terms"
    A, B = float(proj[2][2]), float(proj[3][2])
    rng = np.random.default_rng(5)
    worst = 0.0
    for D in np.concatenate([[0.1, 0.5, 1.0, 4.0, 1000.0, 9999.0], rng.uniform(0.2, 400.0, 200)]):
        D = float(f32(D))
        clip = GL.matvec(proj, [rng.uniform(-1, 1) * D, rng.uniform(-1, 1) * D, -D, 1.0])
        assert float(clip[3]) == D
        depth = f32(clip[2] / clip[3])
        inv = float(depth) * float(s) + float(b)
        tol = U * ((2 * abs(A) * D + 3 * abs(B - A * D)) / abs(B) + 1)
        worst = max(worst, abs(inv * D - 1) / tol)
        assert abs(inv * D - 1) <= tol * (1 + 1e-3), D
    print(f"largest error / allowance {worst:.3f}")
    assert float(b) * 10000.0 == pytest.approx(1.0, rel=1e-6), "a cleared pixel (depth bits 0) lies at the far plane"
