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

import raster_cases as RC
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
