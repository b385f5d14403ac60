"""The fragment stage's third cut on the GPU (csrc/svr_device.h struct TriRec, csrc/k_tile.hip, csrc/k_bin.hip):
the record holds edges 1 and 2 unbiased and every reader that decides coverage forms f = g - u itself, the common-case stage
reads thirteen record pieces (inv_area from TriRec::pad2) and runs the LOD chain without its upper range select.  Nothing a caller
sees may move: colour, depth and the counters, bit for bit and count for count against the oracle.

Frames of 96 x 64 (3 x 2 tiles), each named for what it guards:
`edges`   24 cells of 16 x 16 pixels, in each a pair of triangles sharing an edge that runs exactly through pixel centres --
          a diagonal either way, a horizontal and a vertical edge -- in each of the three rotations of the vertex order and
          both windings, so the shared edge is edge 0, 1 and 2 of a record and the top-left rule decides every pixel on it.
          test_reference_frames_hold_their_cases computes the records' F_T1 / F_T2 bits as setup_triangle does and asks for
          all four combinations.
`split`   `edges` with the transparent stack of `stack` over tile (0, 0): 142 transparent triangles make that tile's cost
          (svr_device.h tile_cost: 40 + 142 - 35 = 147 > SPLIT_MIN_COST) enough to be cut into quarters under the default
          tuning, so the shared edges go through the quarter instance of the scan and resolve_record's callers there.
`stack`   70 transparent layers over one 32 x 8 band (a wave's rows of the ordered pass) and, half way, a sliver layer of 3
          pixels: a layer is one chunk of 64 work items, a full group of 64 fragments comes every second row, so the flushes
          fall mid-chunk, and after the sliver on a chunk's last row.  An opaque wall behind half of the band's columns.
`lod`     a common-case material (trilinear, 64 x 64 texels) under five samplers: clamps (0, none), (2, 2), (-1000, 1000),
          and two ranges outside [-50, 50], (60, 1000) and (-1000, -60), which the host marks wide (generic stage).  Under
          each: uv constant over the quad (rho2 = 0), u stepping 2^20 per pixel over a quad 1.5 pixels wide (|u| < 2^23 and
          the sum of the triangle's |u|, |v| under 2^22: the range proofs hold, rho2 = 2^52 saturates to max_lod), the same
          step over 20 pixels (demoted: the generic stage), and an ordinary minified strip.
`reach`   192 x 96, the one frame over 96 x 64: "more than 16 tiles" needs 17 tiles of 32 x 32, 18 here.  Two triangles of 18
          tiles each (the queue of big triangles, k_bin.hip bin_big) sharing a hypotenuse of slope -1/2 through pixel
          centres, their legs along pixel centres too; and a triangle through the near plane (z > w at one corner: the
          clipper's pieces, binned from their own edges) whose edge inside the volume lies on a row of pixel centres, with a
          neighbour sharing that edge.

Each frame in RGBA16F and RGBA8, instrumented and not (an instrumented pass whose hierarchical test would have dropped a
winning fragment -- Counters::hiz_bad -- fails svr_get_stats), under the default tuning, without the split, and with the
hierarchical depth test forced (SVR_OPT_TUNING bit 6); `edges` also under a scissor with an odd origin; and as a depth-only
pass."""
import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu
f32 = np.float32

FORMATS = {"rgba16f": A.COLOR_RGBA16F, "rgba8": A.COLOR_RGBA8}
EMPTY = np.zeros(0, dtype=A.RENDER_OBJECT_DTYPE)
BOUNDS = dict(extents=(1e6, 1e6, 1e6))
CLEAR = (0.25, 0.5, 0.75, 1)
TUNE_NO_SPLIT, TUNE_HIZ = 8, 64  # SVR_OPT_TUNING bits 3 and 6 (csrc/svr_device.h)
TUNINGS = {"split": 0, "unsplit": TUNE_NO_SPLIT, "split_hiz": TUNE_HIZ, "unsplit_hiz": TUNE_HIZ | TUNE_NO_SPLIT}
ODD_SCISSOR = (3, 5, 85, 53)
COUNTS = ("triangle_count", "drawcall_count", "culled_draws")
# (not shaded_fragments: the kernel shades each visible pixel once, the oracle every fragment that passes the depth test)
INSTR_COUNTS = COUNTS + ("rasterized_fragments", "binned_triangles")
SIZES = {"edges": (96, 64), "split": (96, 64), "stack": (96, 64), "lod": (96, 64), "reach": (192, 96)}


def colour_of(k):
    return (0.25 + 0.125 * (k % 7), 0.125 + 0.0625 * (k % 13), 0.5 + 0.03125 * (k % 11), 1)


def mesh_object(r, mat, size, tris, z=0.5, uvs=None, colours=None):
    """tris: triangles of three (px, py) or (px, py, z) corners in pixels (clip w = 1); triangle k carries colour_of(k)"""
    w, h = size
    pos, col = [], []
    for k, t in enumerate(tris):
        for c in t:
            pos.append((2.0 * c[0] / w - 1.0, 2.0 * c[1] / h - 1.0, c[2] if len(c) > 2 else z))
            col.append(colours[k] if colours else colour_of(k))
    n = len(pos)
    uv = uvs if uvs is not None else [(0.5, 0.5)] * n
    mesh = r.upload_mesh(np.arange(n, dtype=np.uint32), SC.make_vertices(pos, [(0.2, 0.9, 0.4)] * n, uv, col))
    return SC.render_object(mesh, mat, 0, n, **BOUNDS)


def white_material(r, pass_type=None):
    img = r.create_image(S.white_1x1(), mipmapped=True)
    return r.write_material(A.PASS_MAIN_COLOR if pass_type is None else pass_type, (1, 1, 1, 1), img, r.create_sampler(**S.SAMPLER_TRILINEAR))


# ---------------------------------------------------------------------------------------------- edges
def edge_pairs():
    """24 pairs of triangles, one per 16 x 16 cell: (kind, rotation, reversed winding) -> two triangles sharing an edge on pixel centres"""
    pairs = []
    cell = 0
    for kind in ("diag_down", "diag_up", "horizontal", "vertical"):
        for rot in range(3):
            for reverse in (False, True):
                ox, oy = 16 * (cell % 6), 16 * (cell // 6)
                cell += 1
                p00, p10, p11, p01 = (ox + 2.5, oy + 2.5), (ox + 13.5, oy + 2.5), (ox + 13.5, oy + 13.5), (ox + 2.5, oy + 13.5)
                if kind == "diag_down":
                    a, b = [p00, p10, p11], [p00, p11, p01]
                elif kind == "diag_up":
                    a, b = [p00, p10, p01], [p10, p11, p01]
                elif kind == "horizontal":
                    l, rr = (ox + 2.5, oy + 8.5), (ox + 13.5, oy + 8.5)
                    a, b = [l, rr, (ox + 8.0, oy + 2.5)], [l, rr, (ox + 8.0, oy + 13.5)]
                else:
                    t, bt = (ox + 8.5, oy + 2.5), (ox + 8.5, oy + 13.5)
                    a, b = [t, bt, (ox + 2.5, oy + 8.0)], [t, bt, (ox + 13.5, oy + 8.0)]
                for tri in (a, b):
                    tri = tri[rot:] + tri[:rot]
                    pairs.append(tri[::-1] if reverse else tri)
    return pairs


def record_flags(tri):
    """F_T1 | F_T2 << 1 of the record setup_triangle makes of the triangle (csrc/svr_device.h: C4 snap, orientation, edges)"""
    X = [int(round(x * 256)) for x, _ in tri]
    Y = [int(round(y * 256)) for _, y in tri]
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    assert area2 != 0
    if area2 < 0:
        X[1], X[2], Y[1], Y[2] = X[2], X[1], Y[2], Y[1]
    flags = 0
    for i in (1, 2):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        if not (dy < 0 or (dy == 0 and dx > 0)):
            flags |= i
    return flags


def edges_frame(r, size):
    return SC.identity_scene(), SC.objs([mesh_object(r, white_material(r), size, edge_pairs())]), EMPTY


# ---------------------------------------------------------------------------------------------- stack
STACK_LAYERS, SLIVER_AT = 70, 35


def stack_objects(r, size, ox, oy):
    """the transparent stack over the band [ox, ox + 32] x [oy + 8, oy + 16]: 70 layers of two triangles, a 3-pixel sliver
    layer half way; depths on either side of 0.5"""
    mt = white_material(r, A.PASS_TRANSPARENT)
    tris, cols = [], []
    for i in range(STACK_LAYERS):
        zi = 0.3 + 0.4 * (i % 11) / 11.0
        c = (0.004 + 0.003 * (i % 5), 0.002 * (i % 3), 0.001 * (i % 7), 1)
        x0, y0, x1, y1 = ox, oy + 8, ox + 32, oy + 16
        tris += [[(x0, y0, zi), (x1, y0, zi), (x1, y1, zi)], [(x0, y0, zi), (x1, y1, zi), (x0, y1, zi)]]
        cols += [c, c]
        if i == SLIVER_AT:
            sx0, sy0, sx1, sy1 = ox + 9, oy + 10, ox + 12, oy + 11  # the pixels (9 .. 11, 10) of the band's tile
            tris += [[(sx0, sy0, 0.7), (sx1, sy0, 0.7), (sx1, sy1, 0.7)], [(sx0, sy0, 0.7), (sx1, sy1, 0.7), (sx0, sy1, 0.7)]]
            cols += [(0.05, 0.0, 0.05, 1)] * 2
    return [mesh_object(r, mt, size, tris, colours=cols)]


def stack_frame(r, size):
    wall = [[(32, 0), (48, 0), (48, 64)], [(32, 0), (48, 64), (32, 64)]]  # opaque, z = 0.5, behind half of the band's columns
    opaque = [mesh_object(r, white_material(r), size, wall, z=0.5, colours=[(0.2, 0.2, 0.2, 1)] * 2)]
    return SC.identity_scene(), SC.objs(opaque), SC.objs(stack_objects(r, size, 32, 0))


def split_frame(r, size):
    scene, opaque, _ = edges_frame(r, size)
    return scene, opaque, SC.objs(stack_objects(r, size, 0, 0))


# ---------------------------------------------------------------------------------------------- lod
LOD_SAMPLERS = [(0.0, A.LOD_CLAMP_NONE), (2.0, 2.0), (-1000.0, 1000.0), (60.0, 1000.0), (-1000.0, -60.0)]
STEP = float(2 ** 20)


def lod_frame(r, size):
    img = r.create_image(S.make_texture(np.random.default_rng(31), 64, 0), mipmapped=True)
    opaque = []
    for j, (lo, hi) in enumerate(LOD_SAMPLERS):  # a row of 12 pixels per sampler
        smp = r.create_sampler(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=lo, max_lod=hi)
        mat = r.write_material(A.PASS_MAIN_COLOR, (0.9, 0.8, 1.0, 1), img, smp)
        y0, y1 = 12 * j + 1, 12 * j + 11
        tris, uvs = [], []

        def quad(x0, x1, u0, u1, v0, v1):
            c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            t = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
            for k in ((0, 1, 2), (0, 2, 3)):
                tris.append([c[i] for i in k])
                uvs.extend(t[i] for i in k)

        quad(2, 22, 0.3, 0.3, 0.7, 0.7)              # uv constant: rho2 = 0
        quad(26.0, 27.5, 0.0, 1.5 * STEP, 0.0, 0.0)  # 2^20 per pixel, common case: covers the column of centres x = 26.5
        quad(32, 52, 0.0, 20 * STEP, 0.0, 0.25)      # the same step over 20 pixels: |u| reaches 2^24, demoted
        quad(56, 94, -0.25, 4.5, -0.25, 1.0)         # minified 8 x: lambda = 3 before the clamp
        opaque.append(mesh_object(r, mat, size, tris, uvs=uvs, colours=[(0.9, 0.8, 1.0, 1)] * len(tris)))
    return SC.identity_scene(), SC.objs(opaque), EMPTY


# ---------------------------------------------------------------------------------------------- reach
def reach_frame(r, size):
    mat = white_material(r)
    big = [[(0.5, 0.5), (180.5, 0.5), (0.5, 90.5)], [(180.5, 0.5), (180.5, 90.5), (0.5, 90.5)]]  # 6 x 3 tiles each; x + 2 y = 181.5 on centres
    # through the near plane (identity viewproj, w = 1: z > 1 is in front of it): the edge y = 40.5 lies inside the volume
    near = [[(20.5, 40.5, 0.75), (150.5, 40.5, 0.75), (90.0, 95.0, 1.5)], [(150.5, 40.5, 0.75), (20.5, 40.5, 0.75), (84.0, 4.0, 0.75)]]
    return SC.identity_scene(), SC.objs([mesh_object(r, mat, size, big, z=0.5), mesh_object(r, mat, size, near)]), EMPTY


FRAMES = {"edges": edges_frame, "split": split_frame, "stack": stack_frame, "lod": lod_frame, "reach": reach_frame}


# ---------------------------------------------------------------------------------------------- rendering
def render(lib, frame, fmt, instrumented, tuning=0, scissor=None):
    size = SIZES[frame]
    r = lib.create(size[0], size[1], fmt)
    scene, opaque, transparent = FRAMES[frame](r, size)
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
    if frame in ("edges", "split"):
        combos = {record_flags(t) for t in edge_pairs()}
        assert combos == {0, 1, 2, 3}, "F_T1 / F_T2 clear and set in all four combinations"
        # diagonal pairs tile their 11 x 11 square of centres (rows and columns 2.5 .. 12.5: the right and bottom edges are out)
        assert st.rasterized_fragments >= int(drawn.sum()) and drawn[2:13, 2:13].all() and not drawn[13, 2:14].any() and not drawn[2:14, 13].any()
    if frame == "edges":
        assert st.rasterized_fragments == int(drawn.sum()), "every pixel once: no overlap, no gap along a shared edge"
    if frame in ("stack", "split"):
        per_layer = 32 * 8
        assert st.triangle_count >= 2 * STACK_LAYERS + 2
        if frame == "stack":
            assert st.rasterized_fragments == 16 * 64 + STACK_LAYERS * per_layer + 3, "the wall, 70 layers of a band, a sliver of 3 pixels"
            assert STACK_LAYERS * per_layer // 2 < st.shaded_fragments - 16 * 64 < STACK_LAYERS * per_layer, "some layers hidden behind the wall"
    if frame == "lod":
        assert drawn[6, 26] and not drawn[6, 25] and not drawn[6, 27], "the 1.5-pixel quads cover one column of centres"
        rows = [ref["color"][12 * j + 6] for j in range(len(LOD_SAMPLERS))]
        assert not np.array_equal(rows[0][60:90], rows[1][60:90]), "the (2, 2) clamp shows on the minified strip"
    if frame == "reach":
        assert st.triangle_count == 4 and st.binned_triangles > 4, "the near plane's triangle arrives as pieces"
        # the legs on the rows and columns of centres 0.5 are top and left edges (in), those on 90.5 and 180.5 bottom and right (out)
        assert drawn[0, 0] and drawn[89, 179] and not drawn[90:, :].any() and not drawn[:, 180:].any() and drawn[41, 21:150].all()
        assert st.rasterized_fragments > 180 * 90 + 2000, "the pair fills its rectangle once; the near plane's pair lies over it"


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_reference_frames_hold_their_cases(oracle, frame, fmt):
    assert_on_its_cases(frame, reference(oracle, frame, FORMATS[fmt]))


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_instance(hip, oracle, frame, fmt, instrumented):
    ref = reference(oracle, frame, FORMATS[fmt])
    for name, tuning in TUNINGS.items():  # (instrumented: svr_get_stats raises if hiz_bad != 0)
        got = render(hip, frame, FORMATS[fmt], instrumented, tuning)
        assert_same(got, ref, f"{frame} {fmt} {name}", instrumented)
    if frame in ("edges", "split"):
        sref = reference(oracle, frame, FORMATS[fmt], ODD_SCISSOR)
        for name in ("split", "unsplit", "split_hiz"):
            got = render(hip, frame, FORMATS[fmt], instrumented, TUNINGS[name], ODD_SCISSOR)
            assert_same(got, sref, f"{frame} {fmt} {name} scissor {ODD_SCISSOR}", instrumented)


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_depth_only_pass(hip, oracle, frame, instrumented):
    ref = reference(oracle, frame, A.COLOR_RGBA16F)
    size = SIZES[frame]
    for name, tuning in TUNINGS.items():
        r = hip.create(size[0], size[1], A.COLOR_RGBA16F)
        scene, opaque, _ = FRAMES[frame](r, size)
        r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
        r.set_option(A.OPT_TUNING, tuning)
        r.draw_depth(scene, opaque)
        r.sync()
        depth, stats = r.read_depth(), r.get_stats()
        r.close()
        T.assert_images_identical(depth, ref["depth"], f"{frame} depth-only {name}")
        if instrumented and frame not in ("stack", "split"):  # (their reference counts the transparent fragments too)
            assert stats.rasterized_fragments == ref["stats"].rasterized_fragments, f"{frame} depth-only {name}: rasterized_fragments"
