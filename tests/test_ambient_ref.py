"""tests/native/ambient_ref.cpp, the scalar reference of the ambient pass (DESIGN C32-C37), pinned without a GPU by closed
forms derived here, the properties of its tap tables, tests/native/light_ref.cpp for the lit colour, and - on random planes
and on two scenes cut from geometry - ambient_ref.ao64, the pass stated in float64 from the definitions, which is shown to
catch twelve wrong variants of the restatement.  `pytest -s` prints the figures of DESIGN.md section 2, family O."""
import subprocess

import numpy as np
import pytest

import ambient_ref as AR
import lighting_ref as LR

f32 = np.float32
IDENTITY = np.eye(4, dtype=f32)
UP = np.array([0, 0, 1, 1], f32)


def flat(w, h, z, normal=UP):
    return np.full((h, w), z, f32), np.broadcast_to(np.asarray(normal, f32), (h, w, 4)).copy()


def test_a_flat_wall_is_open():
    """a constant depth under the identity matrix: every tap's v = Q - P has v.z = 0 exactly, so v . n = 0 with the normal
    (0, 0, 1), every contribution is 0 and a = 1 - coef * 0 = 1; rpx = 0.5 * 16 = 8, so the taps are taken"""
    depth, normal = flat(32, 32, 0.5)
    for flags in (0, AR.NO_BLUR):
        r = AR.run_ref(depth, normal, IDENTITY, radius=0.5, ppu=16.0, intensity=4.0, flags=flags)
        assert (r["kind"] == AR.EVALUATED).all()
        assert np.array_equal(AR.bits(r["out"]), AR.bits(np.ones((32, 32), f32)))
        assert np.array_equal(AR.bits(r["raw"]), AR.bits(np.ones((32, 32, 2), f32)))


def test_a_depth_step_darkens_the_far_side_within_reach():
    """16 x 16 under the identity matrix (P = (xn, yn, z), a pixel is 0.125 wide): columns 0..7 at z = 0.5, columns 8..15
    at z = 0.4375 (reversed Z: further), normal (0, 0, 1), radius 0.25, pixels_per_unit 8: rpx = 2.
    Pixel (8, 8) has rotation 0.  Its taps, |offset| = 2 f_k: k0 0.125 -> (0, 0), skipped; k1 0.875 (1, 1); k2 1.625 (0, 2);
    k3 0.375 -> (0, 0); k4 1.125 (-1, 0); k5 1.875 (-1, -1); k6 0.625 (0, -1); k7 1.375 (1, -1).  Only k4 and k5 land on
    the near side: v = (-0.125, 0, 0.0625) and (-0.125, -0.125, 0.0625), v . n = 0.0625, v . v = 0.01953125 and 0.03515625,
    both below radius^2 = 0.0625.  Every quantity up to there is a power of two or a short sum of them: exact."""
    w = h = 16
    depth, normal = flat(w, h, 0.5)
    depth[:, 8:] = 0.4375
    r = AR.run_ref(depth, normal, IDENTITY, radius=0.25, ppu=8.0, intensity=1.0, flags=AR.NO_BLUR)
    out = r["out"]
    total = f32(0.0) + f32(0.0625) / (f32(0.01953125) + f32(0.0001))
    total = total + f32(0.0625) / (f32(0.03515625) + f32(0.0001))
    want = f32(1.0) - (f32(1.0) * f32(0.25) * f32(0.125)) * total
    assert 0.8 < want < 0.9
    assert AR.bits(out[8, 8]) == AR.bits(want)
    assert AR.bits(r["raw"][8, 8, 0]) == AR.bits(want) and r["raw"][8, 8, 1] == 1.0
    assert (out[:, :8] == 1.0).all(), "the near side sees the far side below its surface"
    assert (out[:, 10:] == 1.0).all(), "beyond the reach of two pixels nothing is seen"
    assert (out[:, 8] < 1.0).all(), "the first column of the far side"


def test_no_intensity_no_occlusion():
    depth, normal, inv_vp, ppu, _ = AR.plane_case(None, 0)
    r = AR.run_ref(depth, normal, inv_vp, ppu=ppu, **dict(AR.PLANE_PARAMS, intensity=0.0))
    assert np.array_equal(AR.bits(r["out"]), AR.bits(np.ones_like(r["out"])))
    assert (r["kind"] >= AR.EVALUATED).any()


def test_below_one_pixel_the_factor_is_one():
    """rpx = radius * ppu / w < 1 for every w of the planes (0.3 and up) at radius 0.005: 0.005 * 47.8 / 0.3 = 0.8"""
    depth, normal, inv_vp, ppu, _ = AR.plane_case(None, 0)
    r = AR.run_ref(depth, normal, inv_vp, ppu=ppu, **dict(AR.PLANE_PARAMS, radius=0.005))
    assert set(np.unique(r["kind"])) == {AR.NO_SURFACE, AR.SMALL}
    assert np.array_equal(AR.bits(r["out"]), AR.bits(np.ones_like(r["out"])))
    assert (r["raw"][..., 1][r["kind"] == AR.SMALL] > 0).all() and (r["raw"][..., 1][r["kind"] == AR.NO_SURFACE] == 0).all()


PERSPECTIVE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], f32)  # h = (xn, yn, 1, z): P = (xn, yn, 1) / z


def test_a_sharp_blur_mixes_nothing_across_a_step():
    """h.w = z under PERSPECTIVE, so the two sides of a step differ in 1/w by 0.0625: the near side (z = 0.5, two units
    away, normal towards the eye) sees the far side behind its surface, so its raw value is exactly 1; the far side's
    first columns are darkened.  With sharpness 0 a near pixel accepts only near taps and stays exactly 1; with
    sharpness 0.5 (0.0625 <= 0.5 * 0.5) it takes the far side's values in"""
    w = h = 16
    depth, normal = flat(w, h, 0.5, (0, 0, -1, 1))
    depth[:, 8:] = 0.4375
    kw = dict(radius=1.0, ppu=8.0, intensity=1.0)
    raw = AR.run_ref(depth, normal, PERSPECTIVE, flags=AR.NO_BLUR, **kw)["out"]
    assert (raw[:, :8] == 1.0).all() and (raw[:, 8] < 1.0).all()
    sharp = AR.run_ref(depth, normal, PERSPECTIVE, sharpness=0.0, **kw)["out"]
    assert (sharp[:, :8] == 1.0).all()
    assert (sharp[:, 8:] >= raw[:, 8:].min()).all() and (sharp[:, 8] < 1.0).all()
    soft = AR.run_ref(depth, normal, PERSPECTIVE, sharpness=0.5, **kw)["out"]
    assert (soft[:, 6:8] < 1.0).all() and (soft[:, :6] == 1.0).all()
    # an interior far pixel under sharpness 0: the mean of the 5 x 3 far taps of its window, summed row-major in fp32
    y, x = 8, 8
    total, count = f32(0.0), 0
    for yy in range(y - 2, y + 3):
        for xx in range(x - 2, x + 3):
            if xx >= 8:
                total, count = total + raw[yy, xx], count + 1
    assert count == 15 and AR.bits(sharp[y, x]) == AR.bits(total / f32(count))


def test_tap_tables():
    """C34: every rotated direction is within 2 ulp of unit length (so |ox|, |oy| <= 16 follows from rpx <= 16 and f < 1),
    the sixteen rotations are distinct angles below 45 degrees, and the fractions are the eight odd sixteenths"""
    D, R, f = AR.tables()
    assert sorted(f.tolist()) == [(2 * i + 1) / 16 for i in range(8)] and f.max() < 1
    assert np.allclose(np.degrees(np.arctan2(D[:, 1].astype(float), D[:, 0].astype(float))) % 360, np.arange(8) * 45, atol=1e-5)
    assert set(np.abs(D).reshape(-1).tolist()) == {0.0, 1.0, float(f32(0.70710678))}
    ang = np.degrees(np.arctan2(R[:, 1].astype(float), R[:, 0].astype(float)))
    assert np.allclose(ang, np.arange(16) * 45 / 16, atol=1e-5)
    assert len({(c, s) for c, s in R.tolist()}) == 16
    ulp = 2.0 ** -23
    for c, s in R:
        for dx, dy in D:
            ux = f32(dx * c) - f32(dy * s)
            uy = f32(float(dx) * float(s) + float(f32(dy * c)))  # fma(dx, s, dy * c): exact in double, rounded once
            assert abs(np.hypot(float(ux), float(uy)) - 1.0) <= 2 * ulp
            assert max(abs(float(ux)), abs(float(uy))) <= 1.0 + 2 * ulp


@pytest.mark.parametrize("scissor", [None, AR.ODD_SCISSOR], ids=["whole", "odd_scissor"])
@pytest.mark.parametrize("flags", [0, AR.NO_BLUR], ids=["blur", "no_blur"])
def test_the_gpu_tests_planes_are_telling(scissor, flags):
    ref = AR.plane_case(scissor, flags)[4]
    AR.assert_plane_case_is_telling(ref, scissor)
    m = AR.inside_of(ref["out"].shape, scissor or (0, 0) + AR.PLANE)
    assert ((ref["out"] >= 0) & (ref["out"] <= 1)).all() and not ref["out"][~m].any()
    if flags:
        assert np.array_equal(AR.bits(ref["out"]), AR.bits(ref["raw"][..., 0]))


def lit_inputs():
    w, h = 48, 40
    rng = np.random.default_rng(7)
    inv_vp, _ = AR.camera(w, h)
    depth, normal = AR.random_gbuffer(w, h, seed=9)
    albedo = rng.uniform(0, 1, (h, w, 4)).astype(f32)
    albedo[..., 3] = np.where(rng.uniform(size=(h, w)) < 0.8, f32(1.0), f32(0.0))
    probe = LR.run_ref(depth, normal, albedo, inv_vp, (0.1,) * 4, (0, 1, 0.5, 1), (1,) * 4)
    ok = probe["winner"] & np.all(np.isfinite(probe["position"]), axis=-1) & (depth > 0)
    ys, xs = np.nonzero(ok)
    pick = rng.integers(0, len(ys), 6)
    lights = np.zeros(6, AR.A.POINT_LIGHT_DTYPE)
    lights["position"] = probe["position"][ys[pick], xs[pick]] + rng.normal(0, 0.05, (6, 3)).astype(f32)
    lights["radius"], lights["color"], lights["intensity"] = 5.0, rng.uniform(0.2, 1, (6, 3)).astype(f32), 2.0
    return depth, normal, albedo, inv_vp, lights


def test_lit_colour_with_an_open_plane_is_light_refs():
    depth, normal, albedo, inv_vp, lights = lit_inputs()
    lighting = ((0.05, 0.2, 0.15, 1.0), (0.6, 0.3, -0.7, 0.0), (1.0, 0.9, 0.8, 0.7))
    want = LR.run_ref(depth, normal, albedo, inv_vp, *lighting, lights=lights)
    got = AR.run_light_ref(depth, normal, albedo, np.ones_like(depth), inv_vp, *lighting, lights=lights)
    assert want["winner"].any() and (want["rgba"][..., :3][want["winner"]] > 0).any()
    for k in ("rgba", "position"):
        assert np.array_equal(AR.bits(got[k]), AR.bits(want[k])), k
    for k in ("winner", "shadowed"):
        assert np.array_equal(got[k], want[k]), k
    # and the factor is the ambient term's alone: without sun weight and lights the colour is (c * ambient) * ao
    ao = np.random.default_rng(3).uniform(0, 1, depth.shape).astype(f32)
    dark = AR.run_light_ref(depth, normal, albedo, ao, inv_vp, lighting[0], lighting[1], (1.0, 0.9, 0.8, 0.0))
    amb = np.array(lighting[0][:3], f32)
    expect = np.where(dark["winner"][..., None], (albedo[..., :3] * amb) * ao[..., None], f32(0))
    assert np.array_equal(AR.bits(dark["rgba"][..., :3]), AR.bits(expect.astype(f32)))


# ---------------------------------------------------------------- the fp64 statement (ambient_ref.ao64)
WHOLE = (0, 0) + AR.PLANE
PLANE_CASES = [(scissor, flags) for scissor in (None, AR.ODD_SCISSOR) for flags in (0, AR.NO_BLUR)]
PLANE_IDS = [f"{'odd_scissor' if s else 'whole'}-{'no_blur' if f else 'blur'}" for s, f in PLANE_CASES]
SCENE_CASES = [(name, flags) for name in AR.SCENES for flags in (0, AR.NO_BLUR)]
SCENE_IDS = [f"{n}-{'no_blur' if f else 'blur'}" for n, f in SCENE_CASES]
WHOLE_SCENE = (0, 0) + AR.SCENE


def held(ref, st, flags, scissor, what):
    """|ref - ao64| <= bound on every compared pixel; prints the largest ratio (recorded in DESIGN.md section 2)"""
    worst, at, beyond = AR.compare64(ref["out"], st, flags, scissor)
    value, tie, bound = AR.view_of(st, flags)
    print(f"{what}: largest |ref - ao64| / bound = {worst:.4f} at (y, x) = {at}: {ref['out'][at]!r} vs {value[at]!r}, bound {bound[at]:.3g}; "
          f"tie share {tie[AR.inside_of(tie.shape, scissor)].mean():.4f}")
    assert beyond == 0, f"{what}: {beyond} compared pixels beyond the bound, the worst {worst:.3g} bounds off at (y, x) = {at}"
    # the planes next to the factor: 1/w within its own chain's error, and the three ways a pixel is taken
    m = AR.inside_of(tie.shape, scissor) & ~st["tie_a"]
    assert np.array_equal(ref["kind"][m] >= AR.EVALUATED, st["rpx"][m] >= 1.0)
    assert np.array_equal(ref["kind"][m] == AR.NO_SURFACE, st["rpx"][m] == 0.0)
    assert np.allclose(ref["raw"][..., 1][m], st["hw"][m], rtol=16 * AR.EPS, atol=0)
    return worst


@pytest.mark.parametrize("scissor,flags", PLANE_CASES, ids=PLANE_IDS)
def test_restatement_against_the_fp64_statement(scissor, flags):
    st = AR.plane_statement(scissor)
    AR.assert_statement_is_telling(st, flags, scissor or WHOLE)  # on the statement alone, before any comparison
    held(AR.plane_case(scissor, flags)[4], st, flags, scissor or WHOLE, "random planes")


@pytest.mark.parametrize("name,flags", SCENE_CASES, ids=SCENE_IDS)
def test_analytic_scenes(name, flags):
    """depth and normals from the geometry, positions= the geometry's own points: pixel-centre sampling, the y direction,
    the matrix layout and C17's reconstruction are held against ray-plane intersections, not against themselves"""
    depth, normal, inv_vp, ppu, positions = AR.analytic_scene(name)
    st = AR.scene_statement(name)
    AR.assert_statement_is_telling(st, flags, WHOLE_SCENE)
    rpx = st["rpx"][depth > 0]
    assert rpx.min() < 1.0 and (rpx == 16.0).any() and ((rpx > 2.0) & (rpx < 12.0)).any(), "rpx runs from below one pixel to the cap"
    ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, flags=flags, **AR.SCENE_PARAMS)
    held(ref, st, flags, WHOLE_SCENE, name)
    floor = (depth > 0) & (normal[..., 1] == 1) & (positions[..., 1] < 0.5 * AR.BOX_TOP)  # (a cut's y is 0 or the top to an ulp)
    if name == "crease":
        wall = (depth > 0) & (normal[..., 1] == 0)
        assert floor.sum() > 1000 and wall.sum() > 1000, "both in view"
        assert (st["a"][floor] < 0.5).any() and (st["a"][wall] < 0.5).any(), "the crease closes both sides"
    else:
        top = (depth > 0) & (normal[..., 1] == 1) & ~floor
        side = (depth > 0) & (normal[..., 1] == 0)
        assert top.sum() > 100 and side.sum() > 300 and len(np.unique(normal[side], axis=0)) == 2, "the top and two sides of the box"
        # nothing lies above the top face, and the floor past the silhouette is below and behind it: open, exactly
        assert (st["a"][top] == 1.0).all() and (ref["raw"][..., 0][top] == 1.0).all()
        # a side is closed only by the floor at its foot: its upper half, more than a radius' reach of the estimator's
        # weight away, stays lighter than the floor at the foot of the box gets
        assert (st["a"][floor] < 0.1).any() and (st["a"][side & (positions[..., 1] > 0.5 * AR.BOX_TOP)] > 0.5).all()


def variant_cases():
    for scissor, flags in PLANE_CASES:
        depth, normal, inv_vp, ppu, _ = AR.plane_case(scissor, flags)
        yield (f"random planes, {PLANE_IDS[PLANE_CASES.index((scissor, flags))]}", depth, normal, inv_vp, ppu, AR.PLANE_PARAMS, scissor, flags,
               AR.plane_statement(scissor))
    for name, flags in SCENE_CASES:
        depth, normal, inv_vp, ppu, _ = AR.analytic_scene(name)
        yield f"{name}, {'no_blur' if flags else 'blur'}", depth, normal, inv_vp, ppu, AR.SCENE_PARAMS, None, flags, AR.scene_statement(name)


def test_variant_zero_is_the_restatement():
    depth, normal, inv_vp, ppu, ref = AR.plane_case(AR.ODD_SCISSOR, 0)
    again = AR.run_ref(depth, normal, inv_vp, ppu=ppu, scissor=AR.ODD_SCISSOR, variant=0, **AR.PLANE_PARAMS)
    for k in ("raw", "out"):
        assert np.array_equal(AR.bits(again[k]), AR.bits(ref[k]))
    with pytest.raises(subprocess.CalledProcessError):  # an unknown variant is refused, not taken as the contract
        AR.run_ref(depth, normal, inv_vp, ppu=ppu, variant=len(AR.WRONG_VARIANTS) + 1, **AR.PLANE_PARAMS)


@pytest.mark.parametrize("variant", sorted(AR.WRONG_VARIANTS), ids=lambda v: AR.WRONG_VARIANTS[v].replace(" ", "_"))
def test_wrong_variant_of_the_restatement_is_caught(variant):
    """caught: it leaves the bound on a compared pixel of at least one case"""
    caught = []
    for what, depth, normal, inv_vp, ppu, params, scissor, flags, st in variant_cases():
        wrong = AR.run_ref(depth, normal, inv_vp, ppu=ppu, flags=flags, scissor=scissor, variant=variant, **params)
        worst, at, beyond = AR.compare64(wrong["out"], st, flags, scissor or (0, 0) + depth.shape[::-1])
        if beyond:
            caught.append(f"{what}: {beyond} pixels, {worst:.3g} bounds off at (y, x) = {at}")
    print(f"variant {variant} ({AR.WRONG_VARIANTS[variant]}) caught by " + ("; ".join(caught) if caught else "nothing"))
    assert caught, AR.WRONG_VARIANTS[variant]


def test_tables_are_their_formulas():
    """C34's literals against the formulas' float64 values rounded once, bit for bit (a cosine of 90 degrees is 0)"""
    D, R, f = AR.tables()
    angle, fraction = AR.tap_formulas()
    once = lambda v: np.where(np.abs(v) < 2.0 ** -40, 0.0, v).astype(f32)
    assert np.array_equal(AR.bits(D), AR.bits(once(np.stack([np.cos(angle[0]), np.sin(angle[0])], axis=-1))))
    assert np.array_equal(AR.bits(R), AR.bits(once(np.stack([np.cos(angle[:, 0]), np.sin(angle[:, 0])], axis=-1))))
    assert np.array_equal(AR.bits(f), AR.bits(fraction.astype(f32))) and np.array_equal(f.astype(np.float64), fraction)
    assert AR.bits(f32(0.70710678)) == AR.bits(f32(np.sqrt(0.5))), "the documented literal is the rounding of the root of a half"


def test_restatement_under_sanitizers():
    """the address and undefined-behaviour sanitizers over the degenerate scissors, a scissor that ends at the last pixel and
    every wrong variant's reads: exit 0 (run_ref checks it), and the plain build's output"""
    exe = AR.ref_exe(sanitize=True)
    depth, normal, inv_vp, ppu, _ = AR.plane_case(None, 0)
    runs = [dict(scissor=s, flags=fl) for s in AR.EDGE_SCISSORS.values() for fl in (0, AR.NO_BLUR)]
    runs += [dict(scissor=(97, 34, 33, 33), flags=0, variant=v) for v in AR.WRONG_VARIANTS]
    for kw in runs:
        plain = AR.run_ref(depth, normal, inv_vp, ppu=ppu, **AR.PLANE_PARAMS, **kw)
        checked = AR.run_ref(depth, normal, inv_vp, ppu=ppu, exe=exe, **AR.PLANE_PARAMS, **kw)
        for k in ("raw", "out", "kind"):
            assert np.array_equal(checked[k].view(np.uint8), plain[k].view(np.uint8)), (kw, k)
    depth, normal, inv_vp, ppu = AR.special_plane()
    plain = AR.run_ref(depth, normal, inv_vp, ppu=ppu, **AR.PLANE_PARAMS)
    checked = AR.run_ref(depth, normal, inv_vp, ppu=ppu, exe=exe, **AR.PLANE_PARAMS)
    assert np.array_equal(AR.bits(checked["out"]), AR.bits(plain["out"])) and np.array_equal(AR.bits(checked["raw"]), AR.bits(plain["raw"]))


def test_behind_the_eye_plane_is_below_one_pixel():
    """h.w < 0 (the matrix of ambient_ref.behind_the_eye): rpx is negative, so the pixel is "below one pixel" and keeps its
    negative 1/w in the raw plane; sharpness hw_c is negative there, so the blur accepts the centre only"""
    depth, normal = AR.plane_case(None, 0)[:2]
    inv_vp, ppu = AR.behind_the_eye(*AR.PLANE)
    for scissor in (None, AR.ODD_SCISSOR):
        r = AR.run_ref(depth, normal, inv_vp, ppu=ppu, scissor=scissor, **AR.PLANE_PARAMS)
        AR.assert_behind_the_eye(r, scissor or WHOLE)


def test_the_statement_offers_its_ties():
    """inputs that sit on a jump exactly: under the identity matrix rpx = 0.5 * 16 = 8, so at a pixel of rotation 0 tap 0
    has rpx f_0 u = (0.5, 0) and tap 2 (0, 6.5): half-integers, a tie, and so is every pixel whose blur accepts it; with
    radius 0.0625, rpx = 1 at every pixel"""
    depth, normal = flat(32, 32, 0.5)
    st = AR.ao64(depth, normal, IDENTITY, radius=0.5, ppu=16.0, intensity=4.0)
    assert st["tie_a"][8, 8] and st["tie_a"][::4, ::4].all() and not st["tie_a"].all()
    assert st["tie_out"][6:11, 6:11].all() and (st["tie_out"] | ~st["tie_a"]).all()
    assert (st["a"] == 1.0).all() and (st["out"] == 1.0).all(), "a flat wall is open"
    assert AR.ao64(depth, normal, IDENTITY, radius=0.0625, ppu=16.0)["tie_a"].all()
    # and one on the range test: the depth step of the closed form above, the radius^2 of tap k5's v . v
    depth[:, 8:] = 0.4375
    kw = dict(ppu=8.0 * 0.25 / np.sqrt(0.03515625), intensity=1.0)
    assert AR.ao64(depth[:16, :16], normal[:16, :16], IDENTITY, radius=np.sqrt(0.03515625), **kw)["tie_a"][8, 8]
