"""tests/native/light_ref.cpp, the reference of the lighting tests, against tests/light_geom_ref.py: the lighting pass
stated from the scene's geometry in float64 (family L).  CPU only.

For every case of tests/light_cases.py the oracle draws the scene and its depth is read back; the NORMAL and ALBEDO planes
are filled from the faces the reference says won (the oracle has no such planes); light_ref.cpp produces positions and
colours from them, and the reference must agree at every winner pixel within its derived allowances.  The eleven wrong
variants of the reference must each disagree, and the worst error over allowance is held in [0.01, 1.0] per quantity:
the allowance is neither slack nor - being made of attainable input errors, like family D's snap term - held under one half.

The checker (`check_colour`, `check_positions`, `check_allowances`) is the one tests/test_light_geom_gpu.py holds the HIP
library to."""
import functools

import numpy as np
import pytest

import ambient_ref as AR
import light_cases as LC
import light_geom_ref as LG
import lighting_ref as LR
import raster_cases as RC

A, GL = LC.A, LC.GL
f32 = np.float32
AO_PARAMS = dict(radius=3.0, bias=0.01, intensity=1.5, sharpness=0.05)
RATIO_BOUNDS = (0.01, 1.0)
ALL = [c.name for c in LC.all_cases()]
BY_NAME = {c.name: c for c in LC.all_cases()}
# the families whose cases exercise a variant (an identity matrix shows neither a transposition nor, with lights placed by
# the reference, anything of the shadow map)
EXERCISED_BY = {"corner_sample": "L1", "window_y_up": "L3", "inverse_transposed": "L3", "linear_falloff": "L1", "no_plus_one": "L1",
                "normalised_normal": "L1", "lights_skip_shadowed": "L3s", "shadow_texel_round": "L3s", "shadow_bias_sign": "L3s",
                "shadow_outside_is_dark": "L3s", "shadowed_is_black": "L3s"}


# ---------------------------------------------------------------- the checker
def check_cap(case, ref, what=""):
    """the either/or rules are offered at no more than 1 % of the case's winner pixels"""
    n = int(ref.winner.sum())
    used = int(ref.offered.sum()) + int(ref.shadow_alt.sum())
    assert n >= LC.MIN_WINNERS and int(case.owned[ref.ys, ref.xs].sum()) >= LC.MIN_WINNERS, f"{case.name}: {n} winner pixels"
    assert used <= RC.EITHER_OR_CAP * n, f"{case.name}{what}: either/or offered at {used} of {n} winner pixels"
    return used


def check_allowances(case, ref):
    """the rounding part of every allowance against the stated multiple of eps times its magnitude sum"""
    assert np.all(ref.tolP["round"] <= LG.K_POSITION * LG.EPS * ref.magP), f"{case.name}: position"
    k = (LG.K_LIGHT + LG.K_SUN + ref.lights)[:, None]
    assert np.all(ref.tol_parts["round"] <= k * LG.EPS * ref.mag), f"{case.name}: colour"


def colour_errors(ref, decoded):
    """error over allowance of the winner pixels (n, 3), the better of the two where the shadow test is offered either way"""
    got = decoded[ref.ys, ref.xs, :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - LG.stored(ref.rgb, ref.fmt)) / ref.tol
        alt = np.abs(got - LG.stored(ref.rgb_alt, ref.fmt)) / ref.tol_alt
    worse = ~(e.max(axis=1) <= alt.max(axis=1))
    e[ref.shadow_alt & worse] = alt[ref.shadow_alt & worse]
    return np.where(np.isfinite(e), e, np.inf)


def check_colour(case, ref, texels, what):
    """texels: a colour target as read back.  -> the worst error over allowance among the owned winner pixels"""
    dec = LG.decode(texels, ref.fmt)
    own = case.owned[ref.ys, ref.xs]
    assert np.all(dec[ref.ys[own], ref.xs[own], 3] == 1.0), f"{case.name} ({what}): alpha of a lit pixel"
    e = colour_errors(ref, dec)[own]
    bad = np.nonzero(e.max(axis=1) > 1.0)[0]
    if len(bad):
        i = np.nonzero(own)[0][bad[0]]
        raise AssertionError(f"{case.name} ({what}): {len(bad)} of {int(own.sum())} owned winner pixels beyond the allowance, first at (y, x) = "
                             f"({ref.ys[i]}, {ref.xs[i]}): {dec[ref.ys[i], ref.xs[i], :3].tolist()} against {ref.rgb[i].tolist()} +- {ref.tol[i].tolist()}")
    return float(e.max())


def check_positions(case, ref, position, what):
    got = position.astype(np.float64)[ref.ys, ref.xs]
    e = np.abs(got - ref.P) / ref.dP
    bad = np.nonzero(~(e.max(axis=1) <= 1.0))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{case.name} ({what}): {len(bad)} positions beyond the allowance, first at (y, x) = ({ref.ys[i]}, {ref.xs[i]}): "
                             f"{got[i].tolist()} against {ref.P[i].tolist()} +- {ref.dP[i].tolist()}")
    return float(e.max())


def planes(case, ref):
    """the NORMAL and ALBEDO planes of the reference's winners (float32; zero texels elsewhere)"""
    normal, albedo = np.zeros((case.height, case.width, 4), f32), np.zeros((case.height, case.width, 4), f32)
    normal[ref.ys, ref.xs, :3], normal[ref.ys, ref.xs, 3] = ref.normal.astype(f32), 1.0
    albedo[ref.ys, ref.xs, :3], albedo[ref.ys, ref.xs, 3] = ref.albedo.astype(f32), 1.0
    return normal, albedo


def ambient_args(case):
    return dict(inv_vp=case.inv_viewproj, ppu=GL.pixels_per_unit(np.asarray(case.scene.proj, f32).reshape(4, 4), case.height), **AO_PARAMS)


# ---------------------------------------------------------------- the cases on the CPU, each once
@functools.lru_cache(maxsize=None)
def geometry(name, lib):
    """the oracle's coverage and depth of a case, and its shadow map"""
    case = BY_NAME[name]
    rig = LC.Rig(lib, case)
    covered, depth = rig.draw()
    rig.close()
    shadow = None
    if case.shadow:
        srig, shadow = LC.shadow_map(lib, case, depth_only=False)
        srig.close()
    return covered, depth, shadow


@functools.lru_cache(maxsize=None)
def cpu_case(name, lib):
    """-> (the true reference, light_ref's result over the planes it fills)"""
    assert LG.WRONG is None
    case = BY_NAME[name]
    covered, depth, shadow = geometry(name, lib)
    ref = true = _true_reference(name, lib)
    normal, albedo = planes(case, true)
    kw = dict(lights=case.lights)
    if case.ao:
        out = AR.run_light_ref(depth, normal, albedo, true.ao_plane, case.inv_viewproj, case.ambient, case.sun_dir, case.sun_color, **kw)
    else:
        if shadow is not None:
            kw.update(shadow=shadow, shadow_vp=LR.m16(LC.shadow_scene(case.shadow).viewproj), bias=LC.SHADOW_BIAS[case.shadow])
        out = LR.run_ref(depth, normal, albedo, case.inv_viewproj, case.ambient, case.sun_dir, case.sun_color, **kw)
    return ref, out


@functools.lru_cache(maxsize=None)
def _true_reference(name, lib):
    assert LG.WRONG is None, "the cached reference is the true one, whichever tests ran before"
    case = BY_NAME[name]
    covered, depth, shadow = geometry(name, lib)
    ao = None
    if case.ao:  # the ambient plane is an input: ambient_ref's over the oracle's depth and the reference's normals
        probe = case.reference()
        ao = AR.run_ref(depth, planes(case, probe)[0], **ambient_args(case))["out"]
        assert (ao[probe.ys, probe.xs] < 1).any(), "the factor must show"
    ref = case.reference(shadow=shadow, ao=ao)
    ref.ao_plane = ao
    # coverage: the oracle's, as a set, but for the pixels a band or a tie leaves open
    assert np.array_equal(covered & ~ref.offered, ref.winner), f"{name}: {int((covered & ~ref.offered != ref.winner).sum())} pixels covered otherwise"
    assert not (covered & ~ref.covered).any()
    return ref


def stored_texels(out, fmt):
    return LR.store(out["rgba"], fmt)


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ALL)
def test_cases_by_the_reference_alone(name):
    """decided before any library runs: enough winner pixels, a light that changes an owned pixel, the lights' clearance, the
    allowances against their magnitude sums, the either/or cap.  (A shadow map and an ambient plane are inputs a library
    draws: those cases are held here without them, and to the cap again with the planes in hand.)"""
    case = BY_NAME[name]
    ref = case.reference()
    check_cap(case, ref)
    check_allowances(case, ref)
    unlit = case.reference(lights=np.zeros(0, A.POINT_LIGHT_DTYPE))
    own = case.owned[ref.ys, ref.xs]
    assert (np.abs(ref.rgb - unlit.rgb) > ref.tol + unlit.tol)[own].any(), "a light must change an owned pixel"
    lp = case.lights["position"].astype(np.float64)
    d = np.linalg.norm(ref.P[:, None, :] - lp[None, :, :], axis=-1)
    assert d[d < case.lights["radius"][None, :]].min() >= LC.LIGHT_CLEARANCE


def test_l4_uses_the_whole_mask():
    case = LC.cases("L4")[0]
    assert len(case.lights) == A.MAX_LIGHTS == 4096 and set(LC.L4_REACHING) <= set(case.reaching.tolist())
    ref = case.reference()
    lp, lr = case.lights["position"].astype(np.float64), case.lights["radius"].astype(np.float64)
    reached = (((ref.P[:, None, :] - lp[None, :, :]) ** 2).sum(-1) < (lr * lr)[None, :]).any(axis=0)
    assert reached[list(LC.L4_REACHING)].all(), "the lights at the mask's first and last bits must reach a pixel"
    assert not reached[np.setdiff1d(np.arange(4096), case.reaching)].any() and 32 <= reached.sum() <= 64


@pytest.mark.parametrize("name", ALL)
def test_light_ref_against_the_geometry(oracle, name):
    case = BY_NAME[name]
    ref, out = cpu_case(name, oracle)
    used = check_cap(case, ref, " (with the map as read back)")
    check_allowances(case, ref)
    assert np.array_equal(out["winner"], ref.winner)
    rp = check_positions(case, ref, out["position"], "light_ref")
    rc = check_colour(case, ref, stored_texels(out, case.fmt), "light_ref")
    if case.shadow:
        # what the camera is there for, counted by the reference: the box's shadow, lit floor, pixels off the map, pixels behind
        q = np.concatenate([ref.P, np.ones((len(ref.P), 1))], axis=1) @ LG.matrix(LC.shadow_scene(case.shadow).viewproj).T
        behind = q[:, 3] <= 0
        with np.errstate(all="ignore"):
            outside = ~behind & (np.abs(q[:, :2] / q[:, 3:4]).max(axis=1) >= 1)
        floor = np.abs(ref.P[:, 1]) < 1e-6
        counts = dict(shadowed=int(ref.shadowed.sum()), lit_floor=int((~ref.shadowed & floor).sum()), outside=int(outside.sum()), behind=int(behind.sum()))
        print(name, counts)
        assert counts["shadowed"] >= 64 and counts["lit_floor"] >= 256
        assert not ref.shadowed[behind | outside].any()
        if case.shadow == "covers_the_frame":
            assert counts["outside"] == 0 and counts["behind"] == 0
        if case.shadow == "partly_outside":
            assert counts["outside"] >= 256 and counts["behind"] == 0
        if case.shadow == "behind_the_light":
            assert counts["behind"] >= 256 and counts["outside"] >= 256
        assert np.array_equal(out["shadowed"][ref.ys, ref.xs][~ref.shadow_alt], ref.shadowed[~ref.shadow_alt])
    print(f"{name}: {int(ref.winner.sum())} winner pixels, either/or at {used}; worst error / allowance: position {rp:.3f}, colour {rc:.3f}")


@pytest.mark.parametrize("variant", LG.VARIANTS)
def test_wrong_variant_of_the_reference_is_caught(oracle, variant, monkeypatch):
    caught = []
    for case in LC.cases(EXERCISED_BY[variant]):
        true, out = cpu_case(case.name, oracle)  # before the variant is switched on: what is cached is the true reference's
        monkeypatch.setattr(LG, "WRONG", variant)
        wrong = case.reference(shadow=geometry(case.name, oracle)[2], ao=true.ao_plane)
        monkeypatch.setattr(LG, "WRONG", None)
        e = colour_errors(wrong, LG.decode(stored_texels(out, case.fmt), case.fmt))[case.owned[wrong.ys, wrong.xs]]
        n = int((e.max(axis=1) > 1.0).sum())
        if n:
            caught.append((case.name, n, float(e.max())))
    print(variant, caught)
    assert caught, f"{variant} agrees with light_ref on every case of {EXERCISED_BY[variant]}"


@pytest.mark.parametrize("which", sorted(LC.SHADOW_CAMERAS))
def test_shadow_bias_follows_its_rule(oracle, which):
    """light_cases.SHADOW_BIAS: the smallest power of two from SHADOW_BIAS_FLOOR up at which the reference offers no more than
    a third of the cap either way"""
    case = next(c for c in LC.cases("L3s") if c.shadow == which)
    shadow = geometry(case.name, oracle)[2]
    bias = LC.SHADOW_BIAS[which]
    assert bias >= LC.SHADOW_BIAS_FLOOR and np.log2(bias) == np.round(np.log2(bias))

    def offered(b):
        ref = case.reference(shadow=shadow, bias=b)
        return int(ref.offered.sum() + ref.shadow_alt.sum()), int(ref.winner.sum())

    used, n = offered(bias)
    below = [offered(b) for b in 2.0 ** np.arange(np.log2(LC.SHADOW_BIAS_FLOOR), np.log2(bias))]
    print(f"{which}: bias 2^{int(np.log2(bias))}: {used} of {n} winner pixels offered either way; at the powers of two below it: {[u for u, _ in below]}")
    assert used <= RC.EITHER_OR_CAP / 3 * n
    assert all(u > RC.EITHER_OR_CAP / 3 * m for u, m in below), "a smaller bias would do"


def test_worst_error_over_allowance(oracle):
    worst = {"position": 0.0, "colour without shadow": 0.0, "colour with shadow": 0.0}
    for name in ALL:
        case = BY_NAME[name]
        ref, out = cpu_case(name, oracle)
        worst["position"] = max(worst["position"], check_positions(case, ref, out["position"], "light_ref"))
        key = "colour with shadow" if case.shadow else "colour without shadow"
        worst[key] = max(worst[key], check_colour(case, ref, stored_texels(out, case.fmt), "light_ref"))
    print("worst error / allowance:", {k: round(v, 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert RATIO_BOUNDS[0] <= v <= RATIO_BOUNDS[1], f"{k}: {v}"
