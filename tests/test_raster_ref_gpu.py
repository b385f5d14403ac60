"""The cases of tests/raster_cases.py through the HIP library, against tests/raster_ref.py: the checker and the allowances
are those of tests/test_raster_ref.py, unchanged.  All four attribute planes are enabled and EVERY covered pixel of BARY
(b1, b2, 1/w), UV, ALBEDO (the fp32 texel), depth and colour is checked; coverage is set equality.  Nothing here comes out
of the CPU oracle."""
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
            if case.pair:
                union = R.check_pair(prev, got)
                want = R.strictly_inside_union(cases[k - 1], case, case.width, case.height)
                assert not (want & ~union).any(), f"{case.name}: a hole on the shared edge"
            prev = got
    finally:
        rig.close()
    print(f"{len(cases)} cases, {total} covered pixels, either/or used at {used}; worst error / allowance: "
          f"{ {k: round(v, 3) for k, v in ratios.items()} }")
    assert total > 0


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
