"""The fog pass's scalar restatement (tests/native/fog_ref.cpp, DESIGN C55-C60) on the CPU: known answers, the restatement
against an fp64 statement of the same march written from include/svr_fog.h's definitions (fog_ref.march64), and the numbered
wrong variants, each of which must be told apart by more than the allowance.

The allowance (u = 2^-24, n = steps), to first order, from the operation counts of C55-C58:
  e_dir  = 16 u (|cam|_1 + 1) / near      a component of the ray's direction: the near-plane point minus the camera cancels
  e_t    = 16 u (|cam|_1 + max_distance)  any distance along a ray (unprojection: a 4-term chain, 1/w, a product, the
                                          difference from the camera, the squares' chain, the root; then the step's products)
  e_y    = max_distance e_dir + e_t       a sample's height
  e_a1   = k e_y + 4 u A1                 the first exponent, k = falloff log2(e), A1 = k (|cam.y - base| + max_distance dy),
                                          dy the largest |dir.y| of a ray through the image (its corners')
  e_sig  = ln2 e_a1 + 2^-23 + u           sigma, relative (C41's stated error is below 2^-23)
  e_dlt  = e_t / t_min + u                delta, relative; t_min the case's smallest t_end
  e_arg  = e_sig + e_dlt + 3 u            the second exponent x_i = sigma_i delta log2(e), relative
A step's a_i = 2^-x_i then has the relative error x_i ln2 e_arg + 2^-23, and T_i = e^-tau_i, the product of i of them and i
roundings, the relative error tau_i e_arg + i (2^-23 + u) with tau_i the optical depth so far.  tau e^-tau <= 1/e, so
  tol_T  = e_arg / e + n (2^-23 + u).
S sums w_i src with w_i = T_i (1 - a_i) = T_i - T_(i+1) and sum w_i <= 1.  T_i's error puts sum w_i (tau_i e_arg + n (2^-23 + u))
into it, at most e_arg + n (2^-23 + u) because sum (e^-tau_i - e^-tau_(i+1)) tau_i <= the integral of tau e^-tau <= 1; a_i's
error puts sum T_(i+1) (x_i ln2 e_arg + 2^-23) <= e_arg + n 2^-23; the difference, the product and the fma add 3 u sum w_i,
and the n roundings of the running sum n u:
  tol_S  = src_max (2 e_arg + n (2^-22 + 2 u) + 3 u) + sun_max ph_max e_ph, with e_ph the phase's relative error
           (1.5 (4 u (1 + g^2 + 2|g|) + 2|g| (3 e_dir + 3 u)) / (1 - |g|)^2 + 4 u) and ph_max = (1 - g^2) / (4 pi (1 - |g|)^3).
Both grow with n and were not tuned; the figures each case prints stand beside them.
A ray whose fp64 march has a sample within e_pos = max_distance e_dir + e_t world units (scaled by the shadow matrix's rows:
margin()) of a texel edge, the map's border or the bias comparison is left out; at most 15 % of a case's rays may be."""
import math

import numpy as np
import pytest

import fog_ref as FR

f32 = np.float32
U = 2.0 ** -24
W, H = 24, 16
CAM = FR.Camera(W, H, eye=(0.5, 1.0, 1.5), near=0.5)
M_LIGHT, SUN = FR.ortho_light(center=(0.0, 0.0, -12.0), half=32.0, height=80.0)
COARSE = FR.slab_map(8, M_LIGHT, seed=11)  # 8 x 8 texels of 8 world units over the scene
BASE = dict(density=0.05, height_falloff=0.1, height_base=-2.0, max_distance=40.0, fog_color=(0.5, 0.6, 0.7), sun_dir=SUN,
            sun_color=(6.0, 5.0, 4.0), anisotropy=0.4, shadow_bias=0.02, edge_sharpness=4.0, frame_index=5)


def allowance(n, p, t_min, cam=CAM):
    cam1 = float(np.abs(cam.eye).sum())
    e_dir = 16 * U * (cam1 + 1) / cam.near
    e_t = 16 * U * (cam1 + p["max_distance"])
    e_y = p["max_distance"] * e_dir + e_t
    k = p["height_falloff"] * math.log2(math.e)
    a1 = k * (abs(float(cam.eye[1]) - p["height_base"]) + p["max_distance"] * cam.max_dir_y())
    assert a1 < 16 and p["density"] * 2.0 ** a1 * p["max_distance"] / n * math.log2(math.e) < 16, "the case must stay inside C41's range"
    e_sig = math.log(2) * (k * e_y + 4 * U * a1) + 2.0 ** -23 + U
    e_arg = e_sig + e_t / t_min + U + 3 * U
    g = abs(p["anisotropy"])
    ph_max = (1 - g * g) / (4 * math.pi * (1 - g) ** 3)
    e_ph = 1.5 * (4 * U * (1 + g * g + 2 * g) + 2 * g * (3 * e_dir + 3 * U)) / (1 - g) ** 2 + 4 * U
    sun_max, src_max = max(p["sun_color"]), max(p["fog_color"]) + max(p["sun_color"]) * ph_max
    return dict(T=e_arg / math.e + n * (2.0 ** -23 + U), S=src_max * (2 * e_arg + n * (2.0 ** -22 + 2 * U) + 3 * U) + sun_max * ph_max * e_ph,
                t=e_t, e_pos=p["max_distance"] * e_dir + e_t)


def margin(e_pos, n_texels=8):
    """how near a decision boundary a sample may come: (texels to an edge, depth units to the bias comparison)"""
    rows = np.abs(M_LIGHT[:, :3]).sum(axis=1)
    return 0.5 * n_texels * max(rows[0], rows[1]) * e_pos + 4 * U * n_texels, rows[2] * e_pos + 4 * U * (1 + abs(BASE["shadow_bias"]))


def scene(seed=3):
    return FR.random_hdr(W, H, seed), CAM.depth_of(FR.rolling_depth(W, H, seed + 1))


# ---------------------------------------------------------------- known answers
def test_uniform_fog_closed_form():
    """falloff 0, no sun: T = exp(-density t) per block, whatever the steps; where every t is max_distance the upsample mixes
    equal taps and colour = I T + fog_color (1 - T).  Tolerance: T's relative error is n roundings of the product and n
    polynomials (3 n u) plus the exponents' three roundings scaled by the optical depth tau (4 tau u); the colour adds the
    upsample's and the composite's ten roundings and the half's 2^-11."""
    color = FR.random_hdr(W, H, 7)
    p = dict(BASE, height_falloff=0.0, sun_color=(0.0, 0.0, 0.0), density=0.07)
    for steps in (1, 5, 64):
        r = FR.run_ref(color, CAM.depth_of(np.full((H, W), 12.0)), CAM.inv, CAM.eye, steps=steps, **p)
        tau = f32(p["density"]).astype(np.float64) * r["t_end"].astype(np.float64)
        want = np.exp(-tau)
        rel = np.abs(r["st"][..., 3] - want) / want
        print(f"steps {steps}: T's relative error {rel.max():.3g}, allowed {(3 * steps + 4 * tau.max()) * U:.3g}")
        assert (rel <= (3 * steps + 4 * tau) * U).all()
        fog = np.asarray(p["fog_color"], f32).astype(np.float64)
        assert (np.abs(r["st"][..., :3] - fog * (1 - want[..., None])) <= (3 * steps + 4 * tau[..., None] + 2 * steps) * U).all()
        # every pixel beyond max_distance: one T for the whole image
        far = FR.run_ref(color, CAM.depth_of(np.full((H, W), 500.0)), CAM.inv, CAM.eye, steps=steps, **p)
        assert (far["t_end"] == f32(p["max_distance"])).all()
        T = math.exp(-float(f32(p["density"])) * float(f32(p["max_distance"])))
        want_c = FR.floats(color)[..., :3].astype(np.float64) * T + fog * (1 - T)
        got_c = FR.floats(far["color"])[..., :3].astype(np.float64)
        tol = want_c * (2.0 ** -11 + (3 * steps + 4 * tau.max() + 10) * U) + 2.0 ** -24
        print(f"steps {steps}: colour error {np.abs(got_c - want_c).max():.3g}")
        assert (np.abs(got_c - want_c) <= tol).all()
        assert np.array_equal(far["color"][..., 3], color[..., 3])


def test_one_step_closed_form():
    """steps = 1 with o pinned to 1/2: the sample sits at t_end / 2, a = exp(-sigma t_end), S = (1 - a) (fog + sun ph), T = a"""
    color, depth = scene()
    p = dict(BASE, density=0.01, max_distance=20.0)  # thin enough for one step to stay inside C41's range
    r = FR.run_ref(color, depth, CAM.inv, CAM.eye, steps=1, pin_o=0.5, **p)
    m = FR.march64(depth, CAM.inv, CAM.eye, steps=1, pin_o=0.5, **p)
    tol = allowance(1, p, m["t_end"].min())
    # the closed form itself, from the fp64 statement's ray set-up only
    Minv = CAM.inv.astype(np.float64).reshape(4, 4).T
    as64 = lambda v: np.asarray(v, f32).astype(np.float64)  # the values the pass is handed
    g, base, fog, sun_c = float(as64(p["anisotropy"])), float(as64(p["height_base"])), as64(p["fog_color"]), as64(p["sun_color"])
    for by, bx in ((0, 0), (3, 7), (7, 11)):
        q = Minv @ np.array([(2 * bx + 1) * 2.0 / W - 1, (2 * by + 1) * 2.0 / H - 1, 1.0, 1.0])
        d = q[:3] / q[3] - CAM.eye.astype(np.float64)
        d /= np.linalg.norm(d)
        t_end = m["t_end"][by, bx]
        y = float(CAM.eye[1]) + 0.5 * t_end * d[1]
        sigma = float(f32(p["density"])) * math.exp(-float(f32(p["height_falloff"])) * (y - base))
        a = math.exp(-sigma * t_end)
        x = 1 + g * g - 2 * g * d[1]  # the sun is straight up
        ph = (1 - g * g) / (4 * math.pi * x * math.sqrt(x))
        S = (1 - a) * (fog + sun_c * ph)
        assert abs(r["st"][by, bx, 3] - a) <= tol["T"] and (np.abs(r["st"][by, bx, :3] - S) <= tol["S"]).all(), (by, bx)
    assert (np.abs(r["st"][..., 3] - m["T"]) <= tol["T"]).all() and (np.abs(r["st"][..., :3] - m["S"]) <= tol["S"]).all()


def test_density_zero_is_the_identity_on_bits():
    color = FR.random_hdr(W, H, 13, specials=True)
    assert (color == 0x7e00).any() and (color == 0x7c00).any() and (color == 0xfc00).any()
    _, depth = scene()
    r = FR.run_ref(color, depth, CAM.inv, CAM.eye, steps=8, **dict(BASE, density=0.0))
    assert np.array_equal(r["color"], color)
    assert (r["st"][..., :3] == 0).all() and (r["st"][..., 3] == 1).all()
    assert not np.array_equal(FR.run_ref(color, depth, CAM.inv, CAM.eye, steps=8, **BASE)["color"], color)


# ---------------------------------------------------------------- the restatement against the fp64 statement
def compare(r, m, tol, with_map):
    me, mg = margin(tol["e_pos"])
    safe = (m["edge"] > me) & (m["gap"] > mg) if with_map else np.ones(m["T"].shape, bool)
    out = dict(left_out=1.0 - safe.mean(), T=np.abs(r["st"][..., 3] - m["T"])[safe].max(), S=np.abs(r["st"][..., :3] - m["S"])[safe].max(),
               t=np.abs(r["t_end"] - m["t_end"]).max())
    return out


@pytest.mark.parametrize("with_map", [False, True], ids=["no_map", "coarse_map"])
@pytest.mark.parametrize("steps", [4, 16, 64])
def test_against_the_fp64_statement(steps, with_map):
    color, depth = scene()
    kw = dict(BASE, steps=steps, **(dict(shadow_viewproj=FR.colmajor(M_LIGHT)) if with_map else {}))
    shadow = COARSE if with_map else None
    r = FR.run_ref(color, depth, CAM.inv, CAM.eye, shadow=shadow, **kw)
    m = FR.march64(depth, CAM.inv, CAM.eye, shadow=shadow, **kw)
    tol = allowance(steps, kw, m["t_end"].min())
    got = compare(r, m, tol, with_map)
    print(f"steps {steps}, map {with_map}: left out {got['left_out']:.3f}; |dT| {got['T']:.3g} of {tol['T']:.3g}, |dS| {got['S']:.3g} of {tol['S']:.3g}, "
          f"|dt_end| {got['t']:.3g} of {tol['t']:.3g}")
    assert got["left_out"] <= 0.15
    assert got["T"] <= tol["T"] and got["S"] <= tol["S"] and got["t"] <= tol["t"]
    if with_map:
        assert (m["gap"] < np.inf).mean() > 0.9 and 0.05 < (np.abs(r["st"][..., :3] - FR.run_ref(color, depth, CAM.inv, CAM.eye, **kw)["st"][..., :3]).max(-1) > 0).mean()


# ---------------------------------------------------------------- the wrong variants
@pytest.mark.parametrize("variant", [1, 2, 3, 5, 6, 7, 8], ids=lambda v: f"{v}_{FR.WRONG_VARIANTS[v].replace(' ', '_')}")
@pytest.mark.parametrize("steps", [16, 64])
def test_march_variants_are_told_apart(variant, steps):
    color, depth = scene()
    kw = dict(BASE, steps=steps, shadow_viewproj=FR.colmajor(M_LIGHT))
    m = FR.march64(depth, CAM.inv, CAM.eye, shadow=COARSE, **kw)
    tol = allowance(steps, kw, m["t_end"].min())
    good = compare(FR.run_ref(color, depth, CAM.inv, CAM.eye, shadow=COARSE, **kw), m, tol, True)
    bad = compare(FR.run_ref(color, depth, CAM.inv, CAM.eye, shadow=COARSE, variant=variant, **kw), m, tol, True)
    assert good["T"] <= tol["T"] and good["S"] <= tol["S"] and good["t"] <= tol["t"]
    print(f"variant {variant}, {steps} steps: |dT| {bad['T']:.3g} of {tol['T']:.3g}, |dS| {bad['S']:.3g} of {tol['S']:.3g}, |dt_end| {bad['t']:.3g} of {tol['t']:.3g}")
    assert bad["T"] > tol["T"] or bad["S"] > tol["S"] or bad["t"] > tol["t"]


def tap_bound(st, t_end, own, other, share):
    """what a pixel whose taps are the blocks `own` (and, with at most `share` of the normalised weight, `other`) can show
    of S: between the smallest and the largest of its own taps, widened by share times the distance to the others"""
    own_v = np.array([st[b][:3] for b in own])
    lo, hi = own_v.min(0), own_v.max(0)
    if other:
        oth = np.array([st[b][:3] for b in other])
        d = np.maximum(np.abs(oth.max(0) - lo), np.abs(oth.min(0) - hi))
        lo, hi = lo - share * d, hi + share * d
    return lo * (1 - 2.0 ** -10) - 2.0 ** -20, hi * (1 + 2.0 ** -10) + 2.0 ** -20


def tap_rows(y, gh):
    """the block rows pixel row y takes its taps from: floor(y / 2 - 1 / 4) and the next, clamped to the grid"""
    fl = math.floor(y / 2 - 0.25)
    return sorted({min(max(fl + k, 0), gh - 1) for k in (0, 1)})


def edge_case(axial, variant):
    """black pixels under heavy uniform fog: the stored colour is S alone"""
    color = np.zeros((H, W, 4), np.uint16)
    kw = dict(BASE, steps=8, height_falloff=0.0, density=0.08, sun_color=(0.0, 0.0, 0.0), edge_sharpness=4.0, max_distance=60.0)
    r = FR.run_ref(color, CAM.depth_of(axial), CAM.inv, CAM.eye, variant=variant, **kw)
    return r, FR.floats(r["color"])[..., :3].astype(np.float64), kw


def test_plain_bilinear_is_told_apart():
    """half near wall (2 units), half far (40): the last near column's far taps hold a quarter of the bilinear weight; divided
    by 1 + 4 |dt| with |dt| > 30 they keep less than 0.25 / 121 / 0.75 of the normalised weight, so the near side does not take
    the far side's fog.  Variant 4 gives them the whole quarter."""
    share = 0.25 / 121 / 0.75
    x = W // 2 - 1  # odd: taps are its own block column (3/4) and the first far one (1/4)
    verdict = {}
    for variant in (0, 4):
        r, S, kw = edge_case(FR.split_wall(W, H), variant)
        assert np.abs(r["t_end"][:, x // 2 + 1] - r["t_end"][:, x // 2]).min() > 30
        assert (r["st"][:, x // 2 + 1, 0] > 4 * r["st"][:, x // 2, 0]).all(), "the far side holds several times the near side's fog"
        ok = True
        for y in range(H):
            rows = tap_rows(y, H // 2)
            lo, hi = tap_bound(r["st"], r["t_end"], [(by, x // 2) for by in rows], [(by, x // 2 + 1) for by in rows], share)
            ok &= bool((S[y, x] >= lo).all() and (S[y, x] <= hi).all())
        verdict[variant] = ok
    assert verdict == {0: True, 4: False}


def test_tap_clamp_off_by_one_is_told_apart():
    """the last two pixel columns a near wall, the rest far: a pixel of the last column has both its horizontal taps clamped to
    the last block column, so it shows the near wall's fog alone.  Variant 9 clamps to the column before, the far wall's."""
    axial = np.full((H, W), 40.0)
    axial[:, W - 2:] = 2.0
    verdict = {}
    for variant in (0, 9):
        r, S, kw = edge_case(axial, variant)
        gw = W // 2
        assert (r["st"][:, gw - 2, 0] > 4 * r["st"][:, gw - 1, 0]).all()
        ok = True
        for y in range(H):
            rows = tap_rows(y, H // 2)
            lo, hi = tap_bound(r["st"], r["t_end"], [(by, gw - 1) for by in rows], [], 0.0)
            ok &= bool((S[y, W - 1] >= lo).all() and (S[y, W - 1] <= hi).all())
        verdict[variant] = ok
    assert verdict == {0: True, 9: False}


def test_every_variant_changes_the_picture():
    color, depth = scene()
    depth = depth.copy()
    kw = dict(BASE, steps=16, shadow_viewproj=FR.colmajor(M_LIGHT))
    good = FR.run_ref(color, depth, CAM.inv, CAM.eye, shadow=COARSE, **kw)["color"]
    for variant in FR.WRONG_VARIANTS:
        assert not np.array_equal(FR.run_ref(color, depth, CAM.inv, CAM.eye, shadow=COARSE, variant=variant, **kw)["color"], good), variant


# ---------------------------------------------------------------- a perspective light: C18's `q.w > 0`
def test_perspective_light_outside_or_behind_is_lit():
    """Under an orthographic light clip w is 1, and C18's `q.w > 0` never decides.  Under FR.spot_light, hung inside the fog,
    a float64 classification of every sample finds each of C18's four outcomes on at least 5 % of them; and on the blocks
    whose samples are all clearly behind the light (w < -0.05) or clearly outside the map (w > 0.05 and more than 0.05 texel
    from it) the restatement with the map gives (S, T) bit-equal to its run without one: a sample outside the map or behind
    the light is lit.  The margins are four orders of magnitude above fp32's error at these coordinates (|q| < 64, u = 2^-24),
    so the fp32 march decides those samples as float64 does."""
    w, h, steps, n = 33, 17, 7, 16
    cam = FR.Camera(w, h)
    color, depth = FR.random_hdr(w, h, 61, specials=True), cam.depth_of(FR.rolling_depth(w, h, 62))
    M, sun = FR.spot_light()
    smap = FR.spot_map(n, seed=5)
    p = dict(BASE, density=0.06, height_falloff=0.15, height_base=1.0, max_distance=45.0, sun_dir=sun, shadow_bias=0.002, edge_sharpness=2.0,
             frame_index=3, steps=steps)
    pos = FR.sample_points64(depth, cam.inv, cam.eye, steps, p["frame_index"], p["max_distance"])
    q = np.concatenate([pos, np.ones(pos.shape[:-1] + (1,))], -1) @ FR.colmajor(M).astype(np.float64).reshape(4, 4)
    qw = q[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v, sz = (q[..., 0] / qw * 0.5 + 0.5) * n, (q[..., 1] / qw * 0.5 + 0.5) * n, q[..., 2] / qw
    behind = qw <= 0
    inside = ~behind & (np.floor(u) >= 0) & (np.floor(u) < n) & (np.floor(v) >= 0) & (np.floor(v) < n)
    texel = smap.astype(np.float64)[np.clip(np.floor(v), 0, n - 1).astype(int), np.clip(np.floor(u), 0, n - 1).astype(int)]
    dark = inside & (sz + float(f32(p["shadow_bias"])) < texel)
    shares = {"behind the light": behind.mean(), "outside the map": (~behind & ~inside).mean(), "inside, lit": (inside & ~dark).mean(),
              "inside, shadowed": dark.mean()}
    print(", ".join(f"{k} {s:.3f}" for k, s in shares.items()))
    assert all(s >= 0.05 for s in shares.values()), shares

    clearly_behind = qw < -0.05
    clearly_outside = (qw > 0.05) & ((u < -0.05) | (u > n + 0.05) | (v < -0.05) | (v > n + 0.05))
    blocks = (clearly_behind | clearly_outside).all(-1)
    print(f"{int(blocks.sum())} of {blocks.size} blocks qualify, {int((blocks & clearly_behind.any(-1)).sum())} of them hold a behind sample")
    assert blocks.sum() >= 20 and (blocks & clearly_behind.any(-1)).sum() >= 10
    with_map = FR.run_ref(color, depth, cam.inv, cam.eye, shadow=smap, shadow_viewproj=FR.colmajor(M), **p)
    without = FR.run_ref(color, depth, cam.inv, cam.eye, **p)
    assert np.array_equal(with_map["st"][blocks].view(np.uint32), without["st"][blocks].view(np.uint32))
    assert not np.array_equal(with_map["st"][~blocks].view(np.uint32), without["st"][~blocks].view(np.uint32)), "elsewhere the map must matter"
