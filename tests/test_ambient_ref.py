"""tests/native/ambient_ref.cpp, the scalar reference of the ambient pass (DESIGN C32-C37), pinned without a GPU by closed
forms derived here, the properties of its tap tables, and tests/native/light_ref.cpp for the lit colour."""
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
