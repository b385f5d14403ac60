"""The lighting pass of the HIP library (k_light.hip) against tests/light_geom_ref.py, the pass stated
from the scene's geometry in float64: the cases of tests/light_cases.py through svr_draw_geometry with the NORMAL and
ALBEDO planes enabled, then svr_light_pass.  The checker and the allowances are those of tests/test_light_geom_ref.py,
unchanged; nothing here comes out of tests/native/light_ref.cpp but L4's bit-for-bit frame.

Every owned winner pixel of the colour target must lie within the reference's allowance, every other pixel must keep the
pattern it held, the G-buffer planes the pass reads must be the reference's normals and albedo within their allowances, and
the per-tile light counts must lie between the lights that reach a surface point of the tile and those near its box - the
surface points being the reference's, not a reconstruction."""
import functools

import numpy as np
import pytest

import light_cases as LC
import lighting_ref as LR
import test_light_geom_ref as R

A = LC.A
pytestmark = pytest.mark.gpu
GBUFFER = A.ATTR_NORMAL | A.ATTR_ALBEDO
TILE = 32


def tile_bounds(case, ref, counts):
    """reached <= kept <= near per 32 x 32 tile, as tests/test_lighting_gpu.py bounds them, from the geometric surface points"""
    tw, th = -(-case.width // TILE), -(-case.height // TILE)
    assert counts.shape == (tw * th,)
    lp, lr = case.lights["position"].astype(np.float64), case.lights["radius"].astype(np.float64)
    some = 0
    for ty in range(th):
        for tx in range(tw):
            k = int(counts[ty * tw + tx])
            m = (ref.ys // TILE == ty) & (ref.xs // TILE == tx)
            open_pixels = ref.offered[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE].any()
            if not m.any():
                assert k == 0 or open_pixels, f"tile ({tx}, {ty}) has no winner and kept {k} lights"
                continue
            p, dp = ref.P[m], ref.dP[m]
            d = np.sqrt(((p[:, None, :] - lp[None, :, :]) ** 2).sum(-1)) + np.linalg.norm(dp, axis=1)[:, None]
            reached = (d * d < (lr * lr)[None, :] * (1 - 1e-5)).any(0)  # (the margins keep float32 ties out of the lower bound)
            gap = np.maximum(np.maximum((p - dp).min(0)[None, :] - lp, lp - (p + dp).max(0)[None, :]), 0.0)
            near = np.sqrt((gap ** 2).sum(-1)) <= 1.01 * lr
            assert reached.sum() <= k and (k <= near.sum() or open_pixels), \
                f"tile ({tx}, {ty}) kept {k} lights: at least {int(reached.sum())} reach a surface point, {int(near.sum())} are near its box"
            some += int(reached.sum())
    assert some > 0
    return counts


@functools.lru_cache(maxsize=None)
def gpu_case(name, hip):
    """one case through the HIP library, checked -> {"colour": worst error / allowance, "normal", "albedo", "shadow": bool}"""
    case = R.BY_NAME[name]
    rig = LC.Rig(hip, case)
    r = rig.r
    srig = None
    try:
        r.enable_attributes(GBUFFER)
        covered, depth = rig.draw()
        kw, shadow, ao = dict(lights=case.lights), None, None
        if case.shadow:
            srig, shadow = LC.shadow_map(hip, case, depth_only=True)
            kw.update(shadow_ptr=srig.r.get_targets()[1], shadow_size=LC.SHADOW_SIZE, shadow_bias=LC.SHADOW_BIAS[case.shadow],
                      shadow_viewproj=LR.m16(LC.shadow_scene(case.shadow).viewproj))
        if case.ao:
            a = R.ambient_args(case)
            r.ambient_pass(np.asarray(a["inv_vp"]).reshape(4, 4), a["radius"], a["ppu"], a["bias"], a["intensity"], a["sharpness"], 0)
            ao = r.read_ambient()
            r.set_light_ambient_occlusion(True)
        ref = case.reference(shadow=shadow, ao=ao)
        used = R.check_cap(case, ref, " (with the planes as read back)")
        R.check_allowances(case, ref)
        assert np.array_equal(covered & ~ref.offered, ref.winner) and not (covered & ~ref.covered).any(), f"{name}: coverage"
        if ao is not None:
            assert (ao[ref.ys, ref.xs] < 1).any(), "the factor must show"
        # the planes the pass reads
        out = {}
        for key, attr, want, tol in (("normal", A.ATTR_NORMAL, ref.normal, ref.tol_normal), ("albedo", A.ATTR_ALBEDO, ref.albedo, ref.tol_albedo)):
            plane = r.read_attribute(attr).astype(np.float64)
            e = np.abs(plane[ref.ys, ref.xs, :3] - want)
            assert np.all(e <= tol), f"{name}: the {key} plane, worst error / allowance {float((e / tol).max())}"
            out[key] = float((e / np.maximum(tol, 1e-300)).max())
            if key == "albedo":
                assert np.all(plane[ref.ys, ref.xs, 3] == 1.0)
        r.clear_color(LC.PATTERN)  # the whole frame: what is not owned must keep it
        before = r.read_color()
        if case.scissor:
            r.set_scissor(*case.scissor)
        r.set_row_interleave(*case.interleave)
        r.light_pass(case.inv_viewproj, case.ambient, case.sun_dir, case.sun_color, **kw)
        got = r.read_color()
        out["colour"] = R.check_colour(case, ref, got, "HIP")
        keep = ~case.owned | ~ref.covered
        assert np.array_equal(got[keep], before[keep]), f"{name}: a pixel without a winner, or not owned, changed"
        if case.scissor is None and case.interleave == (1, 0):
            counts = tile_bounds(case, ref, r.read_light_tiles())
            if case.family == "L4":
                assert counts.max() < 256, "culling must drop nearly all of the 4096 lights"
                normal, albedo = r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO)
                bits = LR.run_ref(depth, normal, albedo, case.inv_viewproj, case.ambient, case.sun_dir, case.sun_color, lights=case.lights)
                want = LR.expected_color(before, bits, case.fmt)
                assert np.array_equal(got, want), f"{name}: {int(np.any(got != want, axis=-1).sum())} pixels differ from light_ref bit for bit"
        out["shadow"] = bool(case.shadow)
        print(f"{name}: {int(ref.winner.sum())} winner pixels, either/or at {used}; worst error / allowance: colour {out['colour']:.3f}, "
              f"normal plane {out['normal']:.3f}, albedo plane {out['albedo']:.3f}")
        return out
    finally:
        r.close()
        if srig is not None:
            srig.close()


@pytest.mark.parametrize("name", R.ALL)
def test_light_pass_against_the_geometry(hip, name):
    gpu_case(name, hip)


def test_worst_error_over_allowance(hip):
    worst = {"colour without shadow": 0.0, "colour with shadow": 0.0}
    for name in R.ALL:
        out = gpu_case(name, hip)
        key = "colour with shadow" if out["shadow"] else "colour without shadow"
        worst[key] = max(worst[key], out["colour"])
    print("worst error / allowance:", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert R.RATIO_BOUNDS[0] <= v <= R.RATIO_BOUNDS[1], f"{k}: {v}"
