"""The cases of tests/raster_cases.py through the HIP library, against tests/raster_ref.py: the checker and the allowances
are those of tests/test_raster_ref.py, unchanged.  All four attribute planes are enabled and EVERY covered pixel of BARY
(b1, b2, 1/w), UV, ALBEDO (the fp32 texel), depth and colour is checked; coverage is set equality.  Nothing here comes out
of the CPU oracle.

test_clipping adds family D, the clip volume and the guard band: the same checker with the coverage band it has for
triangles that went through the clipper, the parent's perspective-correct values at every covered pixel, and the
fragment count of the instrumented pass against the covered pixels (a pixel drawn twice on a fan's diagonal counts
twice).  With the attribute planes on this runs tile_attr_kernel and the clipper's instance that carries the IDs."""
import numpy as np
import pytest

import image_ref as IR
import raster_cases as RC
import raster_ref as RR
import test_raster_ref as R

pytestmark = pytest.mark.gpu


def run(hip, cases, first=0):
    rig = RC.Rig(hip, cases[0].width, cases[0].height, attributes=True)
    ratios, total, used, prev = R.Ratios(), 0, 0, None
    try:
        for k, case in enumerate(cases):
            got = rig.draw(case)
            n, u = R.check_case(case, RC.reference(case), got, ratios)
            total, used = total + n, used + u
            R.check_pair_of(cases, k, prev, got)
            if getattr(case, "empty", False):
                assert n == 0 and not got["covered"].any() and got["fragments"] == 0, f"{case.name}: something was drawn"
            prev = got
    finally:
        rig.close()
    print(f"{len(cases)} cases, {total} covered pixels, either/or used at {used}; worst error / allowance: "
          f"{ {k: round(v, 3) for k, v in ratios.items()} }")
    if ratios.band_tau:
        print(f"coverage band: worst disagreement {ratios.band_worst:.5f} px from the ideal boundary, tau up to {ratios.band_tau:.5f} px")
    assert total > 0 or all(getattr(c, "empty", False) for c in cases)


@pytest.mark.parametrize("family", ["A32", "A40"])
def test_coverage(hip, family):
    run(hip, RC.cases(family))


def test_interpolation(hip):
    run(hip, RC.cases("B"))


C_GROUPS = ("C-r16x16m", "C-r16x16-", "C-r8x4m", "C-r8x4-", "C-r5x3m", "C-r5x3-", "C-r1x7m", "C-r1x7-", "C-r1x1", "C-exact")


@pytest.mark.parametrize("group", C_GROUPS)
def test_texture_unit(hip, group):
    cases = [c for c in RC.cases("C") if c.name.startswith(group)]
    assert len(cases) in (16, 24, 48)
    run(hip, cases)


def test_every_case_is_in_a_group():
    assert sum(len([c for c in RC.cases("C") if c.name.startswith(g)]) for g in C_GROUPS) == len(RC.cases("C"))
    assert sum(len([c for c in RC.cases("D") if c.group == g]) for g in RC.D_GROUPS) == len(RC.cases("D"))


@pytest.mark.parametrize("group", RC.D_GROUPS)
def test_clipping(hip, group):
    cases = [c for c in RC.cases("D") if c.group == group]
    assert len(cases) >= 12 and (group in ("control", "onplane") or all(c.clipped for c in cases))
    run(hip, cases)


# ---------------------------------------------------------------- the colour target through the other instances
TUNE_NO_SPLIT = 8  # SVR_OPT_TUNING bit 3 (csrc/svr_device.h)
# mode -> (colour format, instrumented, tuning): (a) no attribute planes and no instrumentation is tile_kernel<..., INSTR = false>,
# the instances bench.py times, with and without the tile split; (b) an RGBA8 target
TARGET_MODES = {"timed": (RC.A.COLOR_RGBA16F, False, 0), "timed_unsplit": (RC.A.COLOR_RGBA16F, False, TUNE_NO_SPLIT),
                "rgba8": (RC.A.COLOR_RGBA8, True, 0)}
TARGET_GROUPS = ("A32", "B", "C-r16x16m", "C-r5x3m", "C-exact")


def check_colour_target(case, ref, got, fmt, ratios):
    """coverage as check_case has it for a triangle on the exact path (set equality; covered pixels store alpha 1 over a
    target cleared to alpha 0), depth by check_case's own check, and colour as set membership: raster_ref's texel and its
    allowance plus the colour chain's 7 eps (check_case's), pushed through S1's store for the target's format.
    -> (covered pixels, pixels that needed an alternative)"""
    assert not ref.offered.any() and not ref.clipped.any()
    differ = got["covered"] != ref.covered
    assert not differ.any(), f"{case.name}: coverage differs at {int(differ.sum())} pixels, first (y, x) = {np.argwhere(differ)[0].tolist()}"
    if got["fragments"] is not None and len(case.tris) == 1:
        assert got["fragments"] == int(got["covered"].sum())
    drawn = got["covered"]
    assert not got["depth"][~drawn].any() and not got["color"][~drawn].any(), f"{case.name}: pixels outside the coverage were written"
    n = len(ref.ys)
    if n == 0:
        return 0, 0
    R._check_scalar(case, ref, "depth", np.arange(n), got["depth"][ref.ys, ref.xs], ratios)
    stored = got["color"][ref.ys, ref.xs].astype(np.float64)
    assert np.all(stored[:, 3] == (1.0 if fmt == IR.RGBA16F else 255.0)), f"{case.name}: alpha of a covered pixel is not 1"
    t, tol = ref.val["texel"][:, :3], ref.tol["texel"][:, :3]
    ok = np.all(IR.admissible_np(stored[:, :3], t, tol + 7 * RR.EPS * t, fmt), axis=1)
    # error over what the allowance and the store's half step grant (a half's ulp at the value, or half a byte)
    half_step = R.half_fp16_ulp(t + tol) if fmt == IR.RGBA16F else 0.5 / 255
    value = stored[:, :3] if fmt == IR.RGBA16F else stored[:, :3] / 255.0
    ratios.note("target colour", np.abs(value - np.clip(t, 0, 1 if fmt == IR.RGBA8 else np.inf))[ok], (tol + 7 * RR.EPS * t + half_step)[ok])
    used = 0
    for i in np.nonzero(~ok)[0]:
        alts = ref.alts.get(int(i), [])
        if not any(np.all(IR.admissible_np(stored[i, :3], v[:3], tl[:3] + 7 * RR.EPS * v[:3], fmt)) for v, tl in alts):
            R._fail(case, f"stored colour ({len(alts)} alternatives offered)", i, ref, stored[i, :3], t[i], tol[i])
        used += 1
    offered = int(ref.ambiguous.sum())
    if case.exact:
        assert offered == 0 and used == 0
    assert used <= offered <= R.EITHER_OR_CAP * n, f"{case.name}: either/or offered at {offered} and used at {used} of {n} covered pixels"
    return n, used


@pytest.mark.parametrize("mode", list(TARGET_MODES))
@pytest.mark.parametrize("group", TARGET_GROUPS)
def test_colour_target_through_the_other_instances(hip, group, mode):
    """families A32 and B and three groups of C through the uninstrumented tile kernel (default tuning and unsplit) and
    into an RGBA8 target: instances that the attribute-plane runs above never reach"""
    cases = RC.cases(group) if group in ("A32", "B") else [c for c in RC.cases("C") if c.name.startswith(group)]
    fmt, instrumented, tuning = TARGET_MODES[mode]
    rig = RC.Rig(hip, cases[0].width, cases[0].height, attributes=False, color_format=fmt, instrumented=instrumented, tuning=tuning)
    ratios, total, used = R.Ratios(), 0, 0
    try:
        for case in cases:
            got = rig.draw(case)
            n, u = check_colour_target(case, RC.reference(case), got, fmt, ratios)
            total, used = total + n, used + u
    finally:
        rig.close()
    print(f"{group} {mode}: {len(cases)} cases, {total} covered pixels, either/or used at {used}; worst error / allowance: "
          f"{ {k: round(v, 3) for k, v in ratios.items()} }")
    # (family A samples the white texel: its colour is exactly 1 and its error 0)
    assert total > 0 and ratios["target colour"] <= 1.0 and (group == "A32" or ratios["target colour"] > 0.0)
