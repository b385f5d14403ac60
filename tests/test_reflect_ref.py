"""The reflection pass's scalar restatement (tests/native/reflect_ref.cpp, DESIGN C73-C79) on the CPU: known answers, the
restatement against fp64 statements written from include/svr_reflect.h's definitions (reflect_ref.trace64 and resolve64), in
two stages, and the numbered wrong variants, each of which must be told apart by more than the allowance on rays that were
kept.

The allowances (u = 2^-24), to first order, from the operation counts of C73-C77; reflect_ref.Margins evaluates them per
ray and per sample, with the ray's own magnitudes:
  e_p   = 8 u (|p|_1 + |cam|_1 + |v|)    a component of p (C17: a four-term chain whose terms cancel down to p, 1 / w, a
                                         product) and of v = p - cam
  e_vh  = e_p / |v| + 4 u                a component of v^: the squares' chain, the root, the reciprocal, the product
  e_d   = 1.8 (3 u + e_vh) + 3 u         d = n^ . v^: |n^|_1 and |v^|_1 are at most sqrt 3 < 1.8, a component of n^ carries
                                         3 u (n is stored in fp32: exact), the chain adds 3 u
  e_r   = 2 e_d + e_vh + 8 u             a component of r = fma(-2 d, n^, v^)
  e_h0  = |M_row|_1 e_p + 4 u H          H: the largest partial sum of the row's chain
  e_dh  = |M_row|_1 (e_r + 4 u 1.8)
  e_h(t) = e_h0 + t e_dh + (3 + refine) u t 1.8 |M_row|_1 + u (H + 1.8 t |M_row|_1)
                                         a component of h at t: t = (i + o) delta carries 3 u (delta's quotient, the sum,
                                         the product), each bisection's mid one more; the fma's own rounding last
  e_px  = W / 2 ((e_hx + |hx / hw| e_hw) / hw + 3 u |hx / hw|) + u W     the sample's position, in pixels
  e_q   = q (e_hw / hw + 3 u)            q = hw fma(depth, inv_z_scale, inv_z_bias)
A ray is left out of stage 1 when any of its evaluated samples, the refinement's included, lies within e_px of a pixel edge
(the scissor's border is one), within e_hw of hw = 0, or within e_q of q = 1 or q = 1 + thickness: there fp32 may decide the
other way.  At most 10 % of a case's rays may be left out, at least 5 % of them must hit and at least 5 % miss.  On the
others the hit pixel is the fp64 statement's, and
  e_k   = intensity (5 (e_d + u) + 5 u) + (13 + refine) u
                                         k: m = 1 - sat(-d) carries e_d + u, its fifth power 5 e_m + 3 u, F two more; fd is
                                         t_hit (3 + refine) u, two products and an fma; fe two roundings; three products
  tol   = e_k R + 2 u R                  a colour component k R of the trace texel (R, a half, is exact); e_k + u for k
  e_t   = (4 + refine) u t_hit
Stage 2 holds the final colour to resolve64 fed the restatement's own trace texels, so C78's comparisons are the only
decisions left: a pixel is left out when a tap's ||iz_j - iz_c| - tol iz_c| is within u (|iz_j| + |iz_c| + |iz_j - iz_c| +
tol iz_c), the two fma, the difference and the product; at most 10 % again.  The colour then carries the sum's eight
roundings, the reciprocal, three products and two fma, 16 u of (acc / ws + I), and the store's rounding to a half, 2^-11 of
the value (2^-25 below the halves' normal range).
None of this was tuned; the figures each case prints stand beside the bounds.  The scene (a low wall, a high camera, a
long max_distance) was chosen so that rays leave the image or hit after few samples: the margins grow with t."""
import functools

import numpy as np
import pytest

import native_ref as N
import reflect_ref as RR

f32 = np.float32
U = RR.U
W, H = 48, 32
CAM = RR.Camera(W, H, eye=(0.3, 2.6, 2.0), target=(0.0, 0.4, -4.0), fov_y=0.8)
SCENE = RR.cast(CAM, wall_h=1.2, seed=5)  # normals of seeded lengths: C74 normalises
BASE = dict(max_distance=14.3, thickness=0.1, f0=0.3, intensity=0.9, distance_fade=0.5, edge_width=3.0, depth_tolerance=0.05, frame_index=5)
CASES = [(8, 0), (16, 4), (64, 8)]
SCISSOR = (3, 5, 41, 23)  # odd origin, odd size; its top edge cuts through the wall


@functools.lru_cache(maxsize=None)
def statement(steps, refine, scissor=None):
    return RR.trace64(SCENE, *CAM.args(), scissor=scissor, **dict(BASE, steps=steps, refine=refine))


@functools.lru_cache(maxsize=None)
def restated(steps, refine, scissor=None, variant=0, resolve=0):
    return RR.run_ref(SCENE, *CAM.args(), scissor=scissor, variant=variant, **dict(BASE, steps=steps, refine=refine, resolve=resolve))


def window(a, scissor):
    sx, sy, sw, sh = scissor if scissor else (0, 0, W, H)
    return a[sy:sy + sh, sx:sx + sw]


def stage1(r, m, refine, scissor=None):
    """the restatement's trace texels r against the statement m -> dict(kept: bool [sh, sw], left_out, hit, miss: shares of
    the traced rays, over: the largest error over its allowance on the kept rays, wrong_pixel: kept rays whose hit pixel
    differs, t: the largest t_hit error over e_t)"""
    rays = m["traced"]
    kept = rays & (m["near"] > 1)
    hit = m["hit"][..., 0] >= 0
    e_k = BASE["intensity"] * (5 * (m["e_d"] + U) + 5 * U) + (13 + refine) * U
    rgb = RR.san64(RR.floats(SCENE["color"])[..., :3])
    R = np.where(hit[..., None], rgb[np.maximum(m["hit"][..., 1], 0), np.maximum(m["hit"][..., 0], 0)], 0.0)
    tol = np.concatenate([e_k[..., None] * R + 2 * U * R, (e_k + U)[..., None]], -1) + 1e-300
    over = np.abs(r["trace"].astype(np.float64) - m["trace"]) / tol
    e_t = (4 + refine) * U * m["t_hit"] + 1e-300
    return dict(kept=kept, left_out=1.0 - kept.sum() / rays.sum(), hit=hit[rays].mean(), miss=1.0 - hit[rays].mean(), over=over[kept].max(),
                wrong_pixel=int(((r["hit"] != m["hit"]).any(-1) & kept).sum()), t=(np.abs(r["t_hit"] - m["t_hit"]) / e_t)[kept].max())


def stage2(r, resolve, scissor=None):
    """the restatement's final colour against resolve64 fed its own trace texels -> dict(left_out, over)"""
    z = RR.resolve64(SCENE, r["trace"], CAM.inv_z_scale, CAM.inv_z_bias, scissor=scissor, **dict(BASE, resolve=resolve))
    kept = z["near"] > 1
    got = window(RR.floats(r["color"])[..., :3].astype(np.float64), scissor)
    I = window(RR.san64(RR.floats(SCENE["color"])[..., :3]), scissor)
    mag = np.maximum(z["rgb"], I) + np.abs(r["trace"][..., :3]).astype(np.float64) * 9
    tol = z["rgb"] * 2.0 ** -11 + 2.0 ** -25 + 16 * U * mag
    return dict(left_out=1.0 - kept.mean(), over=(np.abs(got - z["rgb"]) / tol)[kept].max(), kept=kept)


# ---------------------------------------------------------------- known answers
MIRROR = dict(max_distance=14.3, steps=64, refine=8, thickness=0.1, f0=1.0, intensity=1.0, distance_fade=0.0, edge_width=0.0)
# high enough over the floor that no floor pixel spans more view distance than a ray gains in its first step: at a grazing
# camera a ray can stop on its own pixel, which the contract allows and this test is not about
MIRROR_CAM = dict(eye=(0.3, 2.2, 1.0), target=(0.0, 1.0, -6.0))


def mirrored(cam, g, delta, wall_z=-6.0, wall_h=4.0):
    """for the floor pixels of g: where the mirrored view ray meets the wall's plane, float64 [h, w, 3], and whether that
    point and the ray's point one step delta farther both lie over the wall (a pixel's footprint inside its top) and
    project inside the image: the first sample behind the wall then still sees the wall"""
    eye = cam.eye.astype(np.float64)
    r = (g["point"] - eye) * (1.0, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
        t = (wall_z - g["point"][..., 2]) / r[..., 2]
        m = g["point"] + t[..., None] * r
        ok = (g["kind"] == 1) & (t > 0)
        for pt in (m, m + delta * r):
            q = np.concatenate([pt, np.ones(pt.shape[:2] + (1,))], -1) @ cam.M.T
            foot = q[..., 3] * 2.0 / np.linalg.norm(cam.M[1, :3]) / cam.h  # a pixel's height on the wall, world units
            ok &= (q[..., 3] > 0) & (np.abs(q[..., 0]) < q[..., 3] * (1 - 2.0 / cam.w)) & (np.abs(q[..., 1]) < q[..., 3] * (1 - 2.0 / cam.h))
            ok &= (pt[..., 1] > foot) & (pt[..., 1] < wall_h - foot)
    return m, ok, t


def test_mirror_floor_shows_the_stripe_above_it():
    """A mirror floor (f0 = 1, no fades: k = 1) under a wall of colour stripes, no box: a floor pixel whose mirrored point
    lies on the wall and inside the image shows the stripe the mirrored point lies in.  The hit sample lies at most one
    step delta beyond the wall along the ray, in a pixel whose centre was ray-cast: pixels whose mirrored point is within
    delta plus a pixel's footprint on the wall of a stripe edge are left out."""
    cam = RR.Camera(W, H, **MIRROR_CAM)
    g = RR.cast(cam, wall_h=4.0, box=None)
    r = RR.run_ref(g, *cam.args(), **MIRROR)
    delta = MIRROR["max_distance"] / MIRROR["steps"]
    m, on_wall, t = mirrored(cam, g, delta)
    axial = (np.concatenate([m, np.ones(m.shape[:2] + (1,))], -1) @ cam.M.T)[..., 3]
    footprint = axial * 2.0 / (cam.M[0, :3] @ cam.M[0, :3]) ** 0.5 / W
    with np.errstate(invalid="ignore"):
        to_edge = np.abs(m[..., 0] / RR.STRIPE_W - np.round(m[..., 0] / RR.STRIPE_W)) * RR.STRIPE_W
        reach = t + delta < MIRROR["max_distance"]
        check = on_wall & (to_edge > delta + footprint) & reach
    print(f"{int(check.sum())} floor pixels checked of {int((g['kind'] == 1).sum())}, stripes seen: {sorted(set(RR.stripe_of(m[check][:, 0])))}")
    assert check.sum() >= 150 and len(set(RR.stripe_of(m[check][:, 0]))) >= 3
    want = RR.STRIPES[RR.stripe_of(m[check][:, 0])]
    assert np.array_equal(r["trace"][check][:, 3], np.ones(int(check.sum()), f32)), "k = 1"
    assert np.array_equal(r["trace"][check][:, :3].astype(np.float64), want)
    assert np.array_equal(RR.floats(r["color"])[check][:, :3].astype(np.float64), want), "a mirror shows the wall alone"


def test_weight_is_schlicks_closed_form():
    """no fades, intensity 1: k = F = f0 + (1 - f0) (1 - cos)^5 with cos = eye.y / |p - eye| over the floor, within e_k"""
    cam = RR.Camera(W, H, **MIRROR_CAM)
    g = RR.cast(cam, wall_h=4.0, box=None, seed=9)
    p = dict(MIRROR, f0=0.04)
    r = RR.run_ref(g, *cam.args(), **p)
    m = RR.trace64(g, *cam.args(), **p)
    hit = (r["hit"][..., 0] >= 0) & (g["kind"] == 1)
    assert hit.sum() >= 200
    cos = float(cam.eye[1]) / np.maximum(np.linalg.norm(g["point"] - cam.eye.astype(np.float64), axis=-1), 1e-9)
    f0 = float(f32(0.04))
    want = f0 + (1 - f0) * (1 - cos) ** 5
    e_k = 5 * (m["e_d"] + U) + 5 * U + (13 + p["refine"]) * U
    err = np.abs(r["trace"][..., 3] - want)
    print(f"k from {want[hit].min():.3f} to {want[hit].max():.3f}; largest error {err[hit].max():.3g}, allowed {e_k[hit].min():.3g} .. {e_k[hit].max():.3g}")
    assert (err[hit] <= e_k[hit]).all() and want[hit].max() > 4 * want[hit].min()


def specials_frame(seed):
    g = dict(SCENE)
    g["color"] = RR.random_hdr(W, H, seed, specials=True)
    g["color"][0, :N.SPECIALS.size, 0] = N.SPECIALS
    return g


def test_intensity_zero_is_the_identity_on_bits():
    g = specials_frame(13)
    assert all((g["color"] == s).any() for s in N.SPECIALS)
    r = RR.run_ref(g, *CAM.args(), **dict(BASE, intensity=0.0))
    assert np.array_equal(r["color"], g["color"]) and (r["trace"] == 0).all()
    assert not np.array_equal(RR.run_ref(g, *CAM.args(), **BASE)["color"], g["color"])


@pytest.mark.parametrize("resolve", [0, 1])
def test_nothing_to_trace_leaves_san_of_the_input(resolve):
    """a frame of sky only, and the scene with no albedo flag set: every trace texel is 0 and the colour leaves as san(input)"""
    g = specials_frame(17)
    want = g["color"].copy()
    want[..., :3] = N.san_bits(g["color"][..., :3])
    sky = dict(g, depth=np.zeros((H, W), f32), albedo=np.zeros((H, W, 4), f32))
    unflagged = dict(g, albedo=np.concatenate([SCENE["albedo"][..., :3], np.full((H, W, 1), f32(0.999))], -1))
    for frame in (sky, unflagged, dict(g, normal=np.zeros((H, W, 4), f32)), dict(g, depth=np.zeros((H, W), f32))):
        r = RR.run_ref(frame, *CAM.args(), **dict(BASE, resolve=resolve))
        assert (r["trace"] == 0).all() and np.array_equal(r["color"], want)


def test_a_ray_leaving_the_scissor_misses():
    """the target's first rows hold floor only (row 0 is the bottom of the view): with those rows as the scissor every ray
    leaves through its far edge, and what lies beyond is not read (a frame whose other rows are poison gives the same bits)"""
    m = statement(16, 4)
    n = int(np.argmin((SCENE["kind"] == 1).all(axis=1)))  # the first row that holds something else
    assert n >= 8
    scissor = (0, 0, W, n)
    assert (window(m["hit"], scissor)[..., 0] >= 0).sum() >= 20, "with the whole image some of these rays hit"
    kw = dict(BASE, steps=16, refine=4)
    r = RR.run_ref(SCENE, *CAM.args(), scissor=scissor, **kw)
    assert (r["trace"] == 0).all() and (r["hit"] == -1).all()
    poisoned = {k: SCENE[k].copy() for k in ("color", "depth", "normal", "albedo")}
    poisoned["color"][n:] = 0x7e00
    poisoned["depth"][n:] = np.nan
    poisoned["normal"][n:] = np.nan
    r1, r2 = (RR.run_ref(g, *CAM.args(), scissor=scissor, **dict(kw, resolve=1)) for g in (SCENE, poisoned))
    assert np.array_equal(r1["color"][:n], r2["color"][:n]) and np.array_equal(r2["color"][n:], poisoned["color"][n:])


def test_zero_thickness_with_every_surface_strictly_in_front_or_behind():
    """thickness = 0 asks for q == 1: a sample is in front of the surface or strictly behind it, never on it"""
    r = restated(16, 4)
    assert (r["hit"][..., 0] >= 0).mean() > 0.05
    thin = RR.run_ref(SCENE, *CAM.args(), **dict(BASE, steps=16, refine=4, thickness=0.0))
    assert (thin["trace"] == 0).all() and (thin["hit"] == -1).all()


# ---------------------------------------------------------------- the restatement against the fp64 statements
@pytest.mark.parametrize("steps,refine", CASES)
def test_trace_against_the_fp64_statement(steps, refine):
    r, m = restated(steps, refine), statement(steps, refine)
    got = stage1(r, m, refine)
    by = (m["near_by"] <= 1)[m["traced"]].mean(0)
    print(f"steps {steps}, refine {refine}: {int(m['traced'].sum())} rays, hit {got['hit']:.3f}, left out {got['left_out']:.4f} "
          f"(hw {by[0]:.4f}, pixel edge {by[1]:.4f}, q {by[2]:.4f}), {m['samples'][m['traced']].mean():.1f} samples a ray; "
          f"error over allowance {got['over']:.3g}, t_hit {got['t']:.3g}")
    assert got["left_out"] <= 0.10
    assert got["hit"] >= 0.05 and got["miss"] >= 0.05
    assert got["wrong_pixel"] == 0 and got["over"] <= 1.0 and got["t"] <= 1.0


@pytest.mark.parametrize("resolve", [0, 1])
@pytest.mark.parametrize("steps,refine", CASES)
def test_colour_against_the_fp64_resolve(steps, refine, resolve):
    got = stage2(restated(steps, refine, resolve=resolve), resolve)
    print(f"steps {steps}, refine {refine}, resolve {resolve}: left out {got['left_out']:.4f}, error over allowance {got['over']:.3g}")
    assert got["left_out"] <= 0.10 and got["over"] <= 1.0
    if resolve:
        a, b = restated(steps, refine, resolve=1)["color"], restated(steps, refine)["color"]
        assert (a != b).any(-1).mean() > 0.05, "the resolve must matter"


# ---------------------------------------------------------------- the wrong variants
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12], ids=lambda v: f"{v}_{RR.WRONG_VARIANTS[v].replace(' ', '_')}")
def test_trace_variants_are_told_apart(variant):
    """inside an odd scissor whose top edge cuts through the wall, with an edge fade, 16 steps and 4 bisections"""
    m = statement(16, 4, SCISSOR)
    good = stage1(restated(16, 4, SCISSOR), m, 4, SCISSOR)
    bad_run = restated(16, 4, SCISSOR, variant=variant)
    bad = stage1(bad_run, m, 4, SCISSOR)
    assert good["left_out"] <= 0.10 and good["over"] <= 1.0 and good["wrong_pixel"] == 0
    n = int(((np.abs(bad_run["trace"] - restated(16, 4, SCISSOR)["trace"]) > 0).any(-1) & good["kept"]).sum())
    print(f"variant {variant}: error over allowance {bad['over']:.3g} (the contract's: {good['over']:.3g}), {n} kept rays differ")
    assert bad["over"] > 1.0


@pytest.mark.parametrize("variant", [10, 11], ids=lambda v: f"{v}_{RR.WRONG_VARIANTS[v].replace(' ', '_')}")
def test_resolve_variants_are_told_apart(variant):
    good = stage2(restated(16, 4, SCISSOR, resolve=1), 1, SCISSOR)
    bad = stage2(restated(16, 4, SCISSOR, variant=variant, resolve=1), 1, SCISSOR)
    print(f"variant {variant}: error over allowance {bad['over']:.3g} (the contract's: {good['over']:.3g})")
    assert good["left_out"] <= 0.10 and good["over"] <= 1.0
    assert np.array_equal(restated(16, 4, SCISSOR, variant=variant, resolve=1)["trace"], restated(16, 4, SCISSOR, resolve=1)["trace"])
    assert bad["over"] > 1.0


def test_every_variant_changes_the_picture():
    good = restated(16, 4, SCISSOR, resolve=1)["color"]
    for variant in RR.WRONG_VARIANTS:
        assert not np.array_equal(restated(16, 4, SCISSOR, variant=variant, resolve=1)["color"], good), variant


def test_the_restatement_is_clean_under_the_sanitizers():
    """one stand-alone run of reflect_ref built with the address and undefined-behaviour sanitizers, over a frame with
    specials in every plane, an odd scissor and the resolve: the same bytes as the plain build's"""
    g = specials_frame(23)
    g["depth"] = g["depth"].copy()
    g["depth"][3, 4:8] = (np.nan, np.inf, -1.0, 1e30)
    g["normal"] = g["normal"].copy()
    g["normal"][5, 2:5, 0] = (np.nan, np.inf, 1e30)
    kw = dict(BASE, steps=64, refine=8, resolve=1)
    plain, checked = RR.run_ref(g, *CAM.args(), scissor=SCISSOR, **kw), RR.run_ref(g, *CAM.args(), scissor=SCISSOR, sanitize=True, **kw)
    for k in ("color", "hit"):
        assert np.array_equal(plain[k], checked[k])
    assert np.array_equal(plain["trace"].view(np.uint32), checked["trace"].view(np.uint32))
