"""Phase A walks each column's covered span (csrc/svr_span.h column_span in csrc/k_tile.hip scan_columns; DESIGN.md section 5
phase A): the rows on which the three edges are >= 0 are found once per work item, exactly, and only those are walked, with no
edge compare.  Nothing a caller sees may move: colour, depth and the instrumented rasterised-fragment count, bit for bit and count
for count against the oracle, through every path that instantiates the scan -- both colour formats, instrumented and not, the
split (quarter) and the unsplit instance, the hierarchical depth test forced on, a depth-only pass, a scissor with an odd origin.

Four frames of 160 x 96 (5 x 3 tiles), each named for what it guards:
`ties`     axis-aligned quads whose edges lie exactly on pixel centres, in abutting pairs (side by side and one above the other,
           across a tile seam), so every pixel is drawn once and the top-left rule decides each tie: horizontal edges whose
           quotient -f / B is an exact integer in every column, vertical edges (B = 0) whose value is 0 down a whole column;
           a right triangle whose hypotenuse runs through pixel centres (an exact integer quotient on a slanted edge); all of
           it again with reversed winding.
`slivers`  a fan of 240 thin triangles around a point inside the tile (2, 1), reaching across its four neighbours: four batches
           in that tile and far more than 128 columns (no bands), every slope from steep to shallow, each triangle under a pixel
           wide near the apex so that most of its columns are empty, and spans that begin or end on the tiles' first and last
           rows where the fan crosses them.
`bands`    large triangles over whole tiles: one or two of them (<= 64 columns: four bands), three or four (65 .. 128: two
           bands), their diagonals running through the band boundaries; and two slivers whose span in some columns is the single
           row 16 (the first row of a band under either cut) and the single row 15 (the last).
`far`      triangles with two vertices thousands of pixels outside the target, inside the guard band, one corner reaching
           in (edge values of large magnitude), and one triangle through the near plane (clipped pieces, keys with the clipper
           bit)."""
import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T
import test_frag_setup_gpu as base

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu
f32 = np.float32

W, H = base.W, base.H
FORMATS = base.FORMATS
EMPTY = base.EMPTY
CLEAR = (0.25, 0.5, 0.75, 1)
TUNE_NO_SPLIT, TUNE_HIZ = 8, 64  # SVR_OPT_TUNING bits 3 and 6 (csrc/svr_device.h), as tests/test_timed_paths_gpu.py forces them
TUNINGS = {"split": 0, "unsplit": TUNE_NO_SPLIT, "split_hiz": TUNE_HIZ, "unsplit_hiz": TUNE_HIZ | TUNE_NO_SPLIT}
ODD_SCISSOR = (3, 5, 117, 59)
COUNTS = ("triangle_count", "drawcall_count", "culled_draws")
INSTR_COUNTS = COUNTS + ("rasterized_fragments", "binned_triangles")


def material(r):
    img = r.create_image(S.white_1x1(), mipmapped=True)
    return r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, r.create_sampler(**S.SAMPLER_TRILINEAR))


def colour_of(k):
    return (0.25 + 0.125 * (k % 7), 0.125 + 0.0625 * (k % 13), 0.5 + 0.03125 * (k % 11), 1)


def triangles_object(r, mat, tris, z, transform=None):
    """tris: triangles of three (px, py) corners, z: a depth each (clip w = 1); triangle k carries colour_of(k)"""
    pos, col = [], []
    for k, (t, zk) in enumerate(zip(tris, z)):
        for px, py in t:
            pos.append(base.clip_xy(px, py) + (zk,))
            col.append(colour_of(k))
    n = len(pos)
    mesh = r.upload_mesh(np.arange(n, dtype=np.uint32), SC.make_vertices(pos, [(0.2, 0.9, 0.4)] * n, [(0.5, 0.5)] * n, col))
    return SC.render_object(mesh, mat, 0, n, transform=transform, **base.BOUNDS)


def rect(x0, y0, x1, y1, reverse=False):
    a, b = [(x0, y0), (x1, y0), (x1, y1)], [(x0, y0), (x1, y1), (x0, y1)]
    return [a[::-1], b[::-1]] if reverse else [a, b]


# ---------------------------------------------------------------------------------------------- the four frames
TIE_RECTS = [(8.5, 8.5, 24.5, 20.5), (24.5, 8.5, 40.5, 20.5), (8.5, 20.5, 24.5, 36.5), (24.5, 20.5, 40.5, 36.5)]  # 16 x 12, 16 x 16
TIE_TRIANGLE = [(8.5, 48.5), (40.5, 48.5), (8.5, 80.5)]  # hypotenuse x + y = 89 through pixel centres


def ties_pixels():
    """what the top-left rule leaves of the abutting rectangles: every pixel once (per winding)"""
    return sum(int((x1 - x0) * (y1 - y0)) for x0, y0, x1, y1 in TIE_RECTS)


def ties_frame(r):
    mat = material(r)
    tris = []
    for reverse, dx in ((False, 0), (True, 80)):
        for x0, y0, x1, y1 in TIE_RECTS:
            tris += rect(x0 + dx, y0, x1 + dx, y1, reverse)
        t = [(x + dx, y) for x, y in TIE_TRIANGLE]
        tris.append(t[::-1] if reverse else t)
    return SC.identity_scene(), SC.objs([triangles_object(r, mat, tris, [0.5] * len(tris))]), EMPTY


FAN, FAN_CENTRE, FAN_RADIUS = 240, (80.3, 48.2), 40.0


def slivers_frame(r):
    mat = material(r)
    tris, z = [], []
    for i in range(FAN):
        a0, a1 = 2 * np.pi * i / FAN, 2 * np.pi * (i + 1.5) / FAN  # neighbours overlap by half their width: depth decides
        tris.append([FAN_CENTRE, (FAN_CENTRE[0] + FAN_RADIUS * np.cos(a0), FAN_CENTRE[1] + FAN_RADIUS * np.sin(a0)),
                     (FAN_CENTRE[0] + FAN_RADIUS * np.cos(a1), FAN_CENTRE[1] + FAN_RADIUS * np.sin(a1))])
        z.append(0.25 + 0.002 * ((i * 7) % FAN))
    return SC.identity_scene(), SC.objs([triangles_object(r, mat, tris, z)]), EMPTY


def bands_frame(r):
    mat = material(r)
    tris = [[(0, 0), (160, 0), (0, 96)], [(160, 0), (160, 96), (0, 96)],  # the frame's two halves: 32 or 64 columns a tile
            [(0, 0), (100, 0), (0, 70)], [(64, 96), (64, 10), (150, 96)],  # a third and a fourth over some of the tiles
            [(2.0, 15.2), (30.0, 16.2), (30.0, 16.9)],  # row 16 alone in its right-hand columns: the first row of a band
            [(34.0, 14.2), (62.0, 15.2), (62.0, 15.9)]]  # row 15 alone: the last row of a band
    z = [0.3, 0.35, 0.4, 0.45, 0.6, 0.65]
    return SC.identity_scene(), SC.objs([triangles_object(r, mat, tris, z)]), EMPTY


def far_frame(r):
    mat = material(r)
    far = [[(-9000.0, -7000.0), (50.3, 40.7), (-3000.0, -12000.0)], [(14000.0, 300.0), (90.6, 30.2), (12000.0, 9000.0)],
           [(-15000.0, 15000.0), (70.1, 60.9), (-2000.0, 16000.0)], [(300.0, -16000.0), (120.4, 50.5), (16000.0, -900.0)]]
    objects = [triangles_object(r, mat, [t], [1.0], transform=base.layer_transform(k)) for k, t in enumerate(far)]
    # through the near plane: the third vertex lies behind the eye (w < 0)
    pos = [(-0.6, -0.7, 1.0), (0.7, -0.5, 1.0), (-0.2 * -0.5, 0.9 * -0.5, -0.5)]
    mesh = r.upload_mesh(np.arange(3, dtype=np.uint32), SC.make_vertices(pos, [(0.2, 0.9, 0.4)] * 3, [(0.5, 0.5)] * 3, [colour_of(5)] * 3))
    objects.append(SC.render_object(mesh, mat, 0, 3, transform=base.layer_transform(4), **base.BOUNDS))
    return base.projective_scene(), SC.objs(objects), EMPTY


FRAMES = {"ties": ties_frame, "slivers": slivers_frame, "bands": bands_frame, "far": far_frame}


# ---------------------------------------------------------------------------------------------- rendering
def render(lib, frame, fmt, instrumented, tuning=0, scissor=None):
    r = lib.create(W, H, fmt)
    scene, opaque, transparent = FRAMES[frame](r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
    r.set_option(A.OPT_TUNING, tuning)
    if scissor:
        r.set_scissor(*scissor)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    out = T._finish(r)
    r.close()
    return out


_ORACLE = {}


def reference(oracle, frame, fmt, scissor=None):
    """the oracle's instrumented frame, rendered once per (frame, format, scissor) and left as it is"""
    key = (frame, fmt, scissor)
    if key not in _ORACLE:
        _ORACLE[key] = render(oracle, frame, fmt, 1, 0, scissor)
    return _ORACLE[key]


def assert_same(got, ref, what, instrumented):
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(got[key], ref[key], f"{what} {key}")
    for f in (INSTR_COUNTS if instrumented else COUNTS):
        assert getattr(got["stats"], f) == getattr(ref["stats"], f), f"{what}: {f}"


def assert_on_its_cases(frame, ref):
    """the reference itself shows that the frame exercises what it is meant to"""
    st, depth = ref["stats"], ref["depth"]
    drawn = depth != 0.0
    if frame == "ties":
        tri_pixels = 32 * 33 // 2  # centres (8.5 + i, 48.5 + j) with i + j <= 31: the hypotenuse's own, i + j = 32, are out (a right/bottom edge)
        assert st.rasterized_fragments == 2 * (ties_pixels() + tri_pixels) == int(drawn.sum()), "every pixel once: no overlap, no gap"
        for dx in (0, 80):
            assert drawn[8:36, 8 + dx:40 + dx].all() and not drawn[8:36, 40 + dx].any() and not drawn[36, 8 + dx:40 + dx].any(), "left/top in, right/bottom out"
            assert not drawn[7, 8 + dx:40 + dx].any() and not drawn[8:36, 7 + dx].any()
    if frame == "slivers":
        assert st.triangle_count == FAN and st.binned_triangles >= FAN - 4 and st.rasterized_fragments > 1.3 * drawn.sum()
        assert drawn[32, 64:96].any() and drawn[63, 64:96].any() and drawn[48, 41:120].all(), "across the tile's first and last row and its neighbours"
    if frame == "bands":
        assert drawn.all() and abs(st.rasterized_fragments - (W * H + 100 * 70 // 2 + 86 * 86 // 2)) < 200, "the two halves, a third, a fourth, two slivers"
        for (x, y), z in (((29, 16), 0.6), ((61, 15), 0.65)):  # a sliver's single row in this column: the band's first, the band's last
            assert depth[y, x] == f32(z) and depth[y - 1, x] != f32(z) and depth[y + 1, x] != f32(z), f"sliver at ({x}, {y})"
    if frame == "far":
        assert st.triangle_count == 5 and st.binned_triangles > 5, "the near plane's triangle arrives as pieces"
        assert drawn[0, 0] and drawn[0, W - 1] and not drawn.all() and len(np.unique(depth)) >= 6, "wedges from the corners in, five layers"


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_reference_frames_hold_their_cases(oracle, frame, fmt):
    assert_on_its_cases(frame, reference(oracle, frame, FORMATS[fmt]))


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_scan_instance(hip, oracle, frame, fmt, instrumented):
    ref = reference(oracle, frame, FORMATS[fmt])
    for name, tuning in TUNINGS.items():  # (instrumented with the test forced: svr_get_stats raises if a dropped triangle would have won)
        got = render(hip, frame, FORMATS[fmt], instrumented, tuning)
        assert_same(got, ref, f"{frame} {fmt} {name}", instrumented)
    sref = reference(oracle, frame, FORMATS[fmt], ODD_SCISSOR)
    for name in ("split", "unsplit"):
        got = render(hip, frame, FORMATS[fmt], instrumented, TUNINGS[name], ODD_SCISSOR)
        assert_same(got, sref, f"{frame} {fmt} {name} scissor {ODD_SCISSOR}", instrumented)


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_depth_only_pass(hip, oracle, frame, instrumented):
    ref = reference(oracle, frame, A.COLOR_RGBA16F)
    for name, tuning in TUNINGS.items():
        r = hip.create(W, H, A.COLOR_RGBA16F)
        scene, opaque, _ = FRAMES[frame](r)
        r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
        r.set_option(A.OPT_TUNING, tuning)
        st = r.draw_depth(scene, opaque)
        r.sync()
        depth, stats = r.read_depth(), r.get_stats()
        r.close()
        T.assert_images_identical(depth, ref["depth"], f"{frame} depth-only {name}")
        if instrumented:
            assert stats.rasterized_fragments == ref["stats"].rasterized_fragments, f"{frame} depth-only {name}: rasterized_fragments"
