"""The UI overlay pass's arithmetic without a GPU: tests/native/overlay_ref.cpp, the scalar restatement of DESIGN C43-C49,
against the independent statement of tests/overlay_stmt.py and against answers derived by hand; and nine wrong painters
(overlay_ref's variants), each of which some check must tell from the contract.

The colour bound against the statement.  Both sides store UNORM8 after every layer, so what they can differ by is
counted in codes.  One layer: the restatement's fp32 chain (two products and an fmaf for the weights, an fmaf pair per
attribute, three fmaf per filtered channel, a product and an fmaf for the blend: under twenty roundings of values of
magnitude at most a few units, so below 1e-5 in all) against the statement's float64 differs by far less than half a
code (1/510), so the two quantisations of one layer over equal stored texels land on the same code or on neighbours: at
most 1.  Further layers: the stored difference d (in codes) enters the next blend multiplied by 1 - a <= 1, so it arrives
as at most d, the layer's own arithmetic adds far below half a code, and rounding two values at most d + epsilon apart
gives codes at most d + 1 apart.  Hence a pixel reached by k fragments differs by at most k codes per channel, and a pixel
reached by none is the same word."""
import numpy as np
import pytest

import overlay_ref as R
import overlay_stmt as S

A = R.A
BIG = [(-60.0, -60.0), (300.0, -60.0), (-60.0, 300.0)]  # covers every image here
BLACK, W, H = 0xff000000, 12, 8


def black(w=W, h=H):
    return np.full((h, w), BLACK, np.uint32)


def bytes_of(img):
    return np.ascontiguousarray(img, dtype=np.uint32).view(np.uint8).reshape(img.shape + (4,)).astype(np.int64)


def rectangle(x0, y0, x1, y1, diagonal, flip, col=0xffffffff):
    """two triangles sharing a diagonal; flip reverses both windings"""
    a, b, c, d = (x0, y0), (x1, y0), (x1, y1), (x0, y1)
    tris = [(a, b, c), (a, c, d)] if diagonal == 0 else [(a, b, d), (b, c, d)]
    rows = []
    for t in tris:
        rows += R.tri(*(t[::-1] if flip else t), col=col)
    return R.make_list(rows)


# ---------------------------------------------------------------- the checks: each takes a variant and says whether it holds
def check_rectangle_on_corners(variant):
    ok = True
    for diagonal in (0, 1):
        for flip in (False, True):
            _, count, _ = R.run_ref(black(), R.RGBA, rectangle(2.0, 3.0, 9.0, 7.0, diagonal, flip), variant)
            want = np.zeros((H, W), np.uint32)
            want[3:7, 2:9] = 1
            ok = ok and np.array_equal(count, want)
    return ok


def check_rectangle_on_centres(variant):
    """edges through pixel centres: the top and left rows of centres belong to it, the bottom and right ones do not"""
    ok = True
    for diagonal in (0, 1):
        for flip in (False, True):
            _, count, _ = R.run_ref(black(), R.RGBA, rectangle(2.5, 1.5, 9.5, 5.5, diagonal, flip), variant)
            want = np.zeros((H, W), np.uint32)
            want[1:5, 2:9] = 1
            ok = ok and np.array_equal(count, want)
    return ok


def check_vertex_on_a_centre(variant):
    _, count, _ = R.run_ref(black(), R.RGBA, R.make_list(R.tri((2.5, 2.5), (6.5, 2.5), (2.5, 6.5))), variant)
    # the right angle sits on pixel (2, 2)'s centre, on a top and a left edge; the other two vertices lie on the hypotenuse
    want = np.zeros((H, W), np.uint32)
    for j in range(2, 6):
        want[j, 2:2 + (6 - j)] = 1  # the hypotenuse x + y = 9 is a bottom-right edge: centres with i + j < 8
    return np.array_equal(count, want) and count[2, 2] == 1 and count[2, 6] == 0 and count[6, 2] == 0


def check_sliver(variant):
    _, count, stats = R.run_ref(black(), R.RGBA, R.make_list(R.tri((0.6, 1.1), (10.4, 1.1), (10.4, 1.4))), variant)
    return not count.any() and stats == {"triangles": 1, "kept": 0, "tiles": 0}


def check_quantised_layers(variant):
    """ten layers of (128, 128, 128) at alpha 1/255 over black.  Stored after each: 0.50196 -> code 1, then
    1 * 254/255 + 0.50196 = 1.498 -> code 1, for ever.  Unrounded, the sum would climb to 5."""
    rows = []
    for _ in range(10):
        rows += R.tri(*BIG, col=R.pack(128, 128, 128, 1))
    img, count, _ = R.run_ref(black(), R.RGBA, R.make_list(rows), variant)
    return bool((count == 10).all() and (img == 0xff010101).all())


def check_order(variant):
    rows = R.tri(*BIG, col=R.pack(255, 0, 0)) + R.tri(*BIG, col=R.pack(0, 255, 0))
    img, _, _ = R.run_ref(black(), R.RGBA, R.make_list(rows), variant)
    return bool((img == 0xff00ff00).all())


def check_order_of_commands(variant):
    rows = R.tri(*BIG, col=R.pack(255, 0, 0)) + R.tri(*BIG, col=R.pack(0, 255, 0))
    cmds = [(R.NO_CLIP, 0, 0, 0, 3), (R.NO_CLIP, 0, 3, 0, 3)]
    img, _, _ = R.run_ref(black(), R.RGBA, R.make_list(rows, cmds=cmds), variant)
    return bool((img == 0xff00ff00).all())


def check_clip_truncates(variant):
    """(2.6, 1.7) .. (9.9, 6.2): x0 = 2, x1 = 2 + (uint)7.3 = 9; y0 = 1, y1 = 1 + (uint)4.5 = 5"""
    lst = R.make_list(R.tri(*BIG), cmds=[((2.6, 1.7, 9.9, 6.2), 0, 0, 0, 3)])
    _, count, _ = R.run_ref(black(), R.RGBA, lst, variant)
    want = np.zeros((H, W), np.uint32)
    want[1:5, 2:9] = 1
    return np.array_equal(count, want)


def check_formats(variant):
    lst = R.make_list(R.tri(*BIG, col=R.pack(255, 0, 0)))
    bgra, _, _ = R.run_ref(black(), R.BGRA, lst, variant)
    rgba, _, _ = R.run_ref(black(), R.RGBA, lst, variant)
    return bool((bgra == 0xffff0000).all() and (rgba == 0xff0000ff).all())


def check_a8(variant):
    """an A8 texel of 128 under opaque white over black: (1, 1, 1, 0.50196) -> 128 in every colour channel"""
    tex = (np.full((1, 1), 128, np.uint8), 1, 1, A.OVERLAY_TEX_A8)
    img, _, _ = R.run_ref(black(), R.RGBA, R.make_list(R.tri(*BIG), textures=[tex]), variant)
    return bool((img == 0xff808080).all())


def check_clamp_to_edge(variant):
    """u = 0 on a 2 x 1 texture (black, white): s = -0.5, both taps are the black texel"""
    texels = np.array([[[0, 0, 0, 255], [255, 255, 255, 255]]], np.uint8)
    lst = R.make_list(R.tri(*BIG, uv=((0.0, 0.5),) * 3), textures=[(texels, 2, 1, A.OVERLAY_TEX_RGBA8)])
    img, _, _ = R.run_ref(np.full((H, W), 0xff123456, np.uint32), R.RGBA, lst, variant)
    return bool((img == BLACK).all())


def check_blend(variant):
    """(255, 0, 0) at alpha 128 over black: 1 * 0.50196 -> 128"""
    img, _, _ = R.run_ref(black(), R.RGBA, R.make_list(R.tri(*BIG, col=R.pack(255, 0, 0, 128))), variant)
    return bool((img == 0xff000080).all())


def statement_scenes():
    tex = [R.random_texture(7, 5, A.OVERLAY_TEX_RGBA8, 1), R.random_texture(7, 5, A.OVERLAY_TEX_A8, 2), R.random_texture(1, 1, A.OVERLAY_TEX_RGBA8, 3)]
    for seed, (dp, sc) in enumerate([((0.0, 0.0), (1.0, 1.0)), ((3.0, -2.0), (1.5, 0.75)), ((-1.25, 0.5), (2.0, 2.0))]):
        rows = R.soup(6, 20, 14, 100 + seed)
        # two wide translucent triangles over each other and over the soup
        rows += R.tri((-3.0, 0.3), (25.2, 2.0), (4.4, 17.0), col=(R.pack(255, 40, 0, 130), R.pack(0, 255, 90, 200), R.pack(10, 20, 255, 60)),
                      uv=((0.0, 0.0), (1.2, 0.1), (0.4, 1.1)))
        rows += R.tri((22.0, 13.0), (1.5, 12.5), (12.0, -4.0), col=(R.pack(200, 200, 0, 255), R.pack(0, 0, 0, 30), R.pack(255, 255, 255, 128)),
                      uv=((0.9, 0.9), (-0.2, 0.5), (0.5, 0.0)))
        cmds = [((-5.0, -5.0, 40.0, 40.0), 0, 0, 0, 9), ((2.6, 1.7, 15.9, 12.2), 1, 0, 9, 9), ((30.0, 3.0, 4.0, 9.0), 0, 0, 0, 3),
                ((1.0, 1.0, 18.5, 11.5), 2, 18, 18, 6)]
        indices = list(range(18)) + [0, 1, 2, 3, 4, 5]
        yield R.make_list(rows, indices=indices, cmds=cmds, textures=tex, display_pos=dp, scale=sc), R.random_image(20, 14, 7 + seed), seed % 2


def check_statement(variant):
    ok = True
    for lst, image, fmt in statement_scenes():
        want, layers = S.paint(image, fmt, lst)
        got, count, _ = R.run_ref(image, fmt, lst, variant)
        ok = ok and np.array_equal(count, layers)
        ok = ok and bool((np.abs(bytes_of(got) - bytes_of(want)) <= layers.astype(np.int64)[..., None]).all())
    return ok


CHECKS = [check_rectangle_on_corners, check_rectangle_on_centres, check_vertex_on_a_centre, check_sliver, check_quantised_layers, check_order,
          check_order_of_commands, check_clip_truncates, check_formats, check_a8, check_clamp_to_edge, check_blend, check_statement]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_overlay_ref_holds(check):
    assert check(0)


@pytest.mark.parametrize("variant", sorted(R.WRONG_VARIANTS), ids=lambda v: R.WRONG_VARIANTS[v].replace(" ", "_"))
def test_wrong_variant_is_caught(variant):
    caught = [c.__name__ for c in CHECKS if c is not check_statement and not c(variant)]
    assert caught, f"no check tells '{R.WRONG_VARIANTS[variant]}' from the contract"


def test_statement_has_layers():
    """the statement scenes do stack fragments, and leave pixels alone"""
    deepest, untouched = 0, 0
    for lst, image, fmt in statement_scenes():
        _, count, _ = R.run_ref(image, fmt, lst)
        deepest, untouched = max(deepest, int(count.max())), untouched + int((count == 0).sum())
    assert deepest >= 2 and untouched > 0


def test_stats_of_the_reference():
    lst = R.make_list(R.tri((1.0, 1.0), (40.0, 1.0), (1.0, 40.0)) + R.tri((2.0, 2.0), (2.0, 2.0), (5.0, 5.0)) + R.tri((-9.0, -9.0), (-5.0, -9.0), (-9.0, -5.0)))
    _, _, stats = R.run_ref(black(70, 45), R.RGBA, lst)
    assert stats == {"triangles": 3, "kept": 1, "tiles": 4}
