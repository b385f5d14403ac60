"""The common-case fragment stage after its second cut (csrc/k_tile.hip shade_pixel<.., COMMON>, csrc/svr_pixel.h
Codec<RGBA16F>::encode; DESIGN.md section 5 phase B): derivatives without their parity selects, clamps as medians, level extents as
exponents, the fp16 pack as two packed conversions, the top-left bias from the flag bit and
the quad partners' edge values by a flipped sign.  Every one of them is meant to be exact, so nothing a caller sees may move:
colour, depth and the traced fragment, bit for bit against the oracle, in both colour formats, instrumented and not, through the
plain, ID, attribute and depth-load instances of the tile kernel and a draw list.

Three frames of 160 x 96, each case named with the item it guards:
`stage`     four cells whose uv gradients have the four sign combinations across x and y, each one quad: the 8x8 blocks off
            its diagonal are of a single triangle (the quads path), those on it are cut by the edge (the partners' chain);
            traced on odd and even columns and rows (derivative selects, partners' signs, top-left bias).  A quad of constant uv
            (rho2 == 0: the LOD's range selects).  A strip in perspective whose footprint is magnified at one end and
            minified at the other, so some waves fetch one level and some two (the second level's two branches).
`textures`  extents 1x1, 2x1, 1x2, 8x4, 1024x4 and 4x1024 under the LOD clamps (0, 1000), (1.5, 3.25), (-2, 0.5) and (2, 2), six
            strips each with lambda below the lower bound, at it, inside, at the upper bound, above it and magnified, uv starting
            at -0.25 or a quarter of the strip's span before the wrap seam (extents by exponent, clamps as medians).  A sampler
            with min_lod > max_lod is refused.
`stores`    patches whose colour components lie just below, exactly on and just above fp16 rounding ties, from the smallest
            denormal half to the overflow into infinity, and six additive layers staggered over a pixel row, so the ordered
            pass decodes and encodes the target once per layer (the fp16 pack)."""
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
EXTENTS = [(1, 1), (2, 1), (1, 2), (8, 4), (1024, 4), (4, 1024)]  # (w, h)
CLAMPS = [(0.0, 1000.0), (1.5, 3.25), (-2.0, 0.5), (2.0, 2.0)]
SIGNS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]


def mesh_of(r, tris, normal, color):
    pos = np.concatenate([np.asarray(p, dtype=f32) for p, _ in tris])
    uv = np.concatenate([np.asarray(t, dtype=f32) for _, t in tris])
    n = len(pos)
    return r.upload_mesh(np.arange(n, dtype=np.uint32), SC.make_vertices(pos, [normal] * n, uv, [color] * n)), n


# ---------------------------------------------------------------------------------------------- the three frames
def stage_frame(r):
    img = r.create_image(S.make_texture(np.random.default_rng(31), 64, 0), mipmapped=True)
    smp = r.create_sampler(**S.SAMPLER_TRILINEAR)
    mat = r.write_material(A.PASS_MAIN_COLOR, (0.9, 0.8, 1.0, 1), img, smp)
    tris, pixels = [], []
    for c, (su, sv) in enumerate(SIGNS):  # cells of 40 x 48; about 2.7 texels a pixel: two levels
        x0 = 40 * c
        uv = lambda X, Y: (su * (1.7 * X / 40 + 0.4 * Y / 48) - 0.25, sv * (2.3 * Y / 48 - 0.3 * X / 40) + 0.1)
        tris += base.quad(x0, 0, x0 + 40, 48, [1.0, 1.3, 1.6, 1.3], [uv(0, 0), uv(40, 0), uv(40, 48), uv(0, 48)])
        pixels += [(x0 + 27, 10), (x0 + 26, 11), (x0 + 20, 25), (x0 + 21, 24)]  # a block of one triangle; on the diagonal
    tris += base.quad(0, 48, 40, 72, 1.0, [(0.3, 0.6)] * 4)  # constant uv under a constant w: the same u, v at every pixel
    pixels.append((13, 58))
    # 1/w falls from 1 to 1/6 along x: u per pixel grows with w * w, from magnified (one level) to minified (two)
    tris += base.quad(40, 48, 120, 72, [1.0, 6.0, 6.0, 1.0], [(-0.05, 0.0), (0.55, 0.0), (0.55, 0.12), (-0.05, 0.12)])
    pixels += [(42, 60), (117, 61)]
    mesh, n = mesh_of(r, tris, (0.2, 0.9, 0.4), (0.8, 0.9, 1.0, 1))
    return base.projective_scene(), SC.objs([SC.render_object(mesh, mat, 0, n, transform=base.layer_transform(0), **base.BOUNDS)]), EMPTY, pixels


def strip_lambdas(lo, hi, levels):
    top = min(hi, levels - 1 + 0.5)  # (a clamp of 1000 is never reached: the chain's own end instead)
    return (lo - 0.7, lo, 0.5 * (lo + top) + 0.1, top, top + 0.7, -1.5)


def textures_frame(r):
    """a cell of 26 x 24 pixels per (extent, clamp), six strips of 4 rows"""
    opaque, pixels = [], []
    for j, (min_lod, max_lod) in enumerate(CLAMPS):
        smp = r.create_sampler(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=min_lod, max_lod=max_lod)
        for i, (tw, th) in enumerate(EXTENTS):
            texels = np.random.default_rng(1000 * tw + th).integers(0, 256, (th, tw, 4), dtype=np.uint8)
            img = r.create_image(texels, mipmapped=True)
            mat = r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, smp)
            levels = int(np.log2(max(tw, th))) + 1
            pos, uv, idx = [], [], []
            for s, lam in enumerate(strip_lambdas(min_lod, max_lod, levels)):
                rho = 2.0 ** lam  # texels per pixel, both ways
                x0, y0, x1, y1 = 26 * i, 24 * j + 4 * s, 26 * i + 26, 24 * j + 4 * s + 4
                su, sv = 26 * rho / tw, 4 * rho / th
                u0, v0 = -min(0.25, 0.25 * su), -min(0.25, 0.25 * sv)
                for (x, y), t in zip(((x0, y0), (x1, y0), (x1, y1), (x0, y1)), ((u0, v0), (u0 + su, v0), (u0 + su, v0 + sv), (u0, v0 + sv))):
                    pos.append(base.clip_xy(x, y) + (0.5,))
                    uv.append(t)
                idx.append(SC.QUAD_IDX + 4 * s)
            mesh = r.upload_mesh(np.concatenate(idx), SC.make_vertices(pos, [(0.3, 0.8, 0.5)] * 24, uv, [(0.9, 0.8, 1.0, 1)] * 24))
            opaque.append(SC.render_object(mesh, mat, 0, 36))
            if (i + j) % 3 == 0:
                pixels.append((26 * i + 7 + j, 24 * j + 4 * ((i + 2 * j) % 6) + 1 + (i & 1)))
    return SC.identity_scene(), SC.objs(opaque), EMPTY, pixels


def tie_values():
    """(below, on, above) for fp32 values exactly halfway between two neighbouring halves"""
    ties = [2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 0.5 + 2.0 ** -12, 0.75 + 3 * 2.0 ** -12, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
            2 + 2.0 ** -10, 1000.25, 65520.0]
    out = []
    for t in ties:
        t = f32(t)
        assert float(t) == float(ties[len(out)])
        out.append((np.nextafter(t, f32(0)), t, np.nextafter(t, f32(np.inf))))
    return out


def stores_frame(r):
    """ambient 1 and a sun of weight 0 under a white 1 x 1 texture: the stage's output is the vertex colour itself"""
    img = r.create_image(S.white_1x1(), mipmapped=True)
    smp = r.create_sampler(**S.SAMPLER_TRILINEAR)
    mo = r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, smp)
    mt = r.write_material(A.PASS_TRANSPARENT, (1, 1, 1, 1), img, smp)
    opaque, transparent, pixels = [], [], []
    quad = lambda x0, y0, x1, y1, z: [base.clip_xy(x, y) + (z,) for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
    for k, (lo, on, hi) in enumerate(tie_values()):  # patches of 16 x 8
        verts = SC.make_vertices(quad(16 * k, 0, 16 * k + 16, 8, 0.5), [(0, 1, 0)] * 4, [(0.5, 0.5)] * 4, [(lo, on, hi, 1)] * 4)
        opaque.append(SC.render_object(r.upload_mesh(SC.QUAD_IDX, verts), mo, 0, 6))
    pixels.append((37, 3))
    # a dark floor, and six additive layers over rows 16..23, layer k from column 16 k on: one to six of them a pixel
    verts = SC.make_vertices(quad(0, 12, W, 40, 0.25), [(0, 1, 0)] * 4, [(0.5, 0.5)] * 4, [(0.0625, 0.03125, 0.015625, 1)] * 4)
    opaque.append(SC.render_object(r.upload_mesh(SC.QUAD_IDX, verts), mo, 0, 6))
    for k in range(6):
        lo, on, hi = tie_values()[3 + k % 4]
        c = (on / f32(8), lo / f32(6), hi / f32(5), 0.5)
        verts = SC.make_vertices(quad(16 * k, 16, W, 24, 0.5 + 0.05 * k), [(0, 1, 0)] * 4, [(0.5, 0.5)] * 4, [c] * 4)
        transparent.append(SC.render_object(r.upload_mesh(SC.QUAD_IDX, verts), mt, 0, 6))
    pixels += [(20, 19), (131, 20)]
    return SC.identity_scene(ambient=1.0, sun_color=(1, 1, 1, 0)), SC.objs(opaque), SC.objs(transparent), pixels


FRAMES = {"stage": stage_frame, "textures": textures_frame, "stores": stores_frame}


# ---------------------------------------------------------------------------------------------- rendering
def plain(lib, frame, fmt, instrumented, traced):
    """the frame through svr_draw_geometry; traced: one more instrumented pass per traced pixel, its trace slots"""
    r = lib.create(W, H, fmt)
    scene, opaque, transparent, pixels = FRAMES[frame](r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    out = T._finish(r)
    out["pixels"], out["traces"] = pixels, []
    if traced:
        r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
        for x, y in pixels:
            r.trace_pixel(x, y)
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, transparent)
            r.sync()
            out["traces"].append(r.read_trace().copy())
    r.close()
    return out


_ORACLE = {}


def reference(oracle, frame, fmt):
    """the oracle's frame and traces, rendered once per (frame, format) and left as they are"""
    if (frame, fmt) not in _ORACLE:
        _ORACLE[(frame, fmt)] = plain(oracle, frame, fmt, 1, True)
    return _ORACLE[(frame, fmt)]


def assert_on_its_cases(frame, fmt, ref):
    """the reference itself shows that the frame exercises what it is meant to"""
    color = ref["color"]
    assert len(np.unique(color.reshape(-1, 4), axis=0)) > (8 if frame == "stores" else W * H // 8), "the frame is drawn at all"
    if frame == "stage":
        with np.errstate(divide="ignore"):  # lambda of the 64 x 64 texture, from the traced derivatives
            lam = [0.5 * np.log2(max((64.0 * t[6]) ** 2 + (64.0 * t[7]) ** 2, (64.0 * t[8]) ** 2 + (64.0 * t[9]) ** 2)) for t in ref["traces"]]
        assert lam[-2] < 0.0 < lam[-1], f"the strip's footprint is magnified at one end and minified at the other: lambda {lam[-2]}, {lam[-1]}"
        assert all(0.5 < v < 3.0 for v in lam[:16]), f"the gradient cells fetch two levels: lambda {lam[:16]}"
        t = ref["traces"][-3]
        assert t[6] == 0.0 and t[7] == 0.0 and t[8] == 0.0 and t[9] == 0.0, "constant uv: every derivative is zero"
        for c, (su, sv) in enumerate(SIGNS):  # dudx and dvdy carry the cell's signs, on every traced parity
            for t in ref["traces"][4 * c:4 * c + 4]:
                assert np.sign(t[6]) == su and np.sign(t[9]) == sv, f"cell {c}: dudx {t[6]}, dvdy {t[9]}"
    if frame == "stores" and fmt == A.COLOR_RGBA16F:
        halves = color.view(np.uint16).reshape(H, W, 4)
        for k, (lo, on, hi) in enumerate(tie_values()):
            below, tie, above = (int(v) for v in halves[3, 16 * k + 5, :3])
            assert above == below + 1 and tie == (below if below % 2 == 0 else above), f"patch {k}: halves {below:#x} {tie:#x} {above:#x} of {lo!r} {on!r} {hi!r}"
        row = halves[19, :, 0]
        assert len({int(row[16 * k + 8]) for k in range(6)}) == 6, "one to six layers a pixel"


def assert_traces(frame, fmt, got, ref):
    for (x, y), a, b in zip(ref["pixels"], got["traces"], ref["traces"]):
        assert b[0] != 0.0, f"{frame}: the traced pixel ({x}, {y}) lies on a triangle"
        a, b = a[base.TRACE_SLOTS], b[base.TRACE_SLOTS]
        differ = (base.bits(a) != base.bits(b)) & ~(np.isnan(a) & np.isnan(b))  # (a NaN's sign and payload are the machine's, not the contract's)
        assert not differ.any(), f"{frame} {fmt}: trace of pixel ({x}, {y}): slots {base.TRACE_SLOTS[differ].tolist()} differ"


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_plain_passes_and_traces(hip, oracle, frame, fmt, instrumented):
    ref = reference(oracle, frame, FORMATS[fmt])
    assert_on_its_cases(frame, FORMATS[fmt], ref)
    got = plain(hip, frame, FORMATS[fmt], instrumented, bool(instrumented))
    base.assert_frame(got, ref, f"{frame} {fmt}")
    if instrumented:
        assert len(got["traces"]) == len(ref["traces"]) > 2
        assert_traces(frame, fmt, got, ref)


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_instance(hip, oracle, frame, fmt, instrumented):
    """a draw list and the ID, attribute and depth-load instances: their colour and depth are the plain pass's"""
    torch = pytest.importorskip("torch")
    ref = reference(oracle, frame, FORMATS[fmt])
    r = hip.create(W, H, FORMATS[fmt])
    scene, opaque, transparent, _ = FRAMES[frame](r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)

    def check(what):
        base.assert_frame(T._finish(r), ref, f"{frame} {fmt} {what}")

    lst = r.create_draw_list(opaque, transparent)
    r.clear_color(CLEAR)
    r.draw_list(scene, lst)
    check("draw list")
    lst.close()

    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    check("ID target")
    r.enable_ids(False)

    r.enable_attributes(A.ATTR_ALL)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    check("attribute targets")
    r.enable_attributes(0)

    # depth load over a depth target of zeros (the clear value): the same frame
    cdt = torch.int16 if FORMATS[fmt] == A.COLOR_RGBA16F else torch.uint8
    color = torch.zeros((H, W, 4), dtype=cdt, device="cuda")
    depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    r.set_depth_load_op(A.DEPTH_LOAD)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    check("depth load")
    r.set_depth_load_op(A.DEPTH_CLEAR)
    r.bind_targets(None, None)
    r.close()


def test_sampler_with_crossed_clamps_is_refused(hip, oracle):
    """(3, 1): svr_create_sampler admits no min_lod above max_lod, so the stage's median never meets such a pair"""
    for lib in (hip, oracle):
        r = lib.create(16, 16, A.COLOR_RGBA16F)
        with pytest.raises(Exception):
            r.create_sampler(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=3.0, max_lod=1.0)
        r.close()
