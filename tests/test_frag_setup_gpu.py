"""What the fragment stage's common case takes from setup (csrc/svr_device.h tex_consts, frag_ranges_ok), on the GPU: the
texture's packed level constants and the per-triangle range proofs that let the specialised stage run without the
reciprocal's window test and the uv guards.  A triangle that fails a proof gives up its key's common-case bit and takes
the generic stage, so nothing a caller sees may tell: colour, depth and the traced fragment, bit for bit against the oracle,
in both colour formats, instrumented and not, through the plain, ID, multiview, attribute, depth-load and draw-list
instances of the tile kernel.

Two frames of 160 x 96.  `textures`: every power-of-two extent of the list under three LOD clamps, each in four strips
whose uv scale puts lambda below 0, inside the chain, just under and above its last level, uv starting at -0.25 (the wrap
seam).  `ranges`: over a common background, pairs of triangles on either side of each proof's limit — slivers 1/256 px wide
whose third corner has a depth of its own, planes that graze their horizon, w scaled by 2^+-40, 2^+-70 and to the ends
of the reciprocal's window, u at 2^22 - 1, 2^20, 2^22, 2^23, infinite and NaN — so 8x8 blocks hold common and
demoted triangles together; a demoted transparent quad between two common ones in the ordered pass; a grazing triangle
beyond the guard band, cut by the clipper into pieces with and without the corner at the horizon.  Which side of the
predicate each triangle is meant for is stated where it is built, and test_triangles_fall_on_their_sides asks the
predicate itself — the header's own code, compiled on the host as in tests/test_frag_setup.py — over the records those
vertices give.  (The clipper's pieces are made on the device and are not asked.)"""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
f32 = np.float32

W, H = 160, 96
FORMATS = {"rgba16f": A.COLOR_RGBA16F, "rgba8": A.COLOR_RGBA8}
EXTENTS = [(1, 1), (2, 2), (8, 4), (4, 8), (16, 16), (1024, 4), (4, 1024), (256, 256)]  # (w, h)
CLAMPS = [(0.0, 1000.0), (1.5, 3.25), (-2.0, 0.5)]
EMPTY = np.zeros(0, dtype=A.RENDER_OBJECT_DTYPE)
BOUNDS = dict(extents=(1e6, 1e6, 1e6))
# the slots both libraries' traces fill (csrc/k_tile.hip shade_pixel, flush_fragments): key, barycentrics, 1/q, uv and its
# derivatives, texel rgb, normal, colour, light, output, the quad partners' barycentrics and reciprocals, the blend
TRACE_SLOTS = np.array([s for s in range(40) if s not in (10, 14)])


def clip_xy(px, py):
    return 2.0 * px / W - 1.0, 2.0 * py / H - 1.0


# ---------------------------------------------------------------------------------------------- the two frames
def textures_frame(r):
    """(scene, opaque, transparent, traced pixels): a cell of 20 x 32 pixels per (extent, clamp), four strips of 8 rows"""
    opaque, pixels = [], []
    for j, (min_lod, max_lod) in enumerate(CLAMPS):
        smp = r.create_sampler(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=min_lod, max_lod=max_lod)
        for i, (tw, th) in enumerate(EXTENTS):
            texels = np.random.default_rng(1000 * tw + th).integers(0, 256, (th, tw, 4), dtype=np.uint8)
            img = r.create_image(texels, mipmapped=True)
            mat = r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, smp)
            levels = int(np.log2(max(tw, th))) + 1
            pos, uv, idx = [], [], []
            for s, lam in enumerate((-1.5, 0.5 * (levels - 1) + 0.3, levels - 1.4, levels + 0.7)):
                rho = 2.0 ** lam  # texels per pixel, both ways
                x0, y0, x1, y1 = 20 * i, 32 * j + 8 * s, 20 * i + 20, 32 * j + 8 * s + 8
                u0, v0, u1, v1 = -0.25, -0.25, -0.25 + 20 * rho / tw, -0.25 + 8 * rho / th
                for (x, y), t in zip(((x0, y0), (x1, y0), (x1, y1), (x0, y1)), ((u0, v0), (u1, v0), (u1, v1), (u0, v1))):
                    pos.append(clip_xy(x, y) + (0.5,))
                    uv.append(t)
                idx.append(SC.QUAD_IDX + 4 * s)
            mesh = r.upload_mesh(np.concatenate(idx), SC.make_vertices(pos, [(0.3, 0.8, 0.5)] * 16, uv, [(0.9, 0.8, 1.0, 1)] * 16))
            opaque.append(SC.render_object(mesh, mat, 0, 24))
            if (i + j) % 3 == 0:
                pixels.append((20 * i + 7 + j, 32 * j + 8 * ((i + j) % 4) + 3))
    return SC.identity_scene(), SC.objs(opaque), EMPTY, pixels


def projective_scene():
    """clip = (x, y, (0.45 + 0.1 k) z, z) for a vertex (x, y, z) of an object whose transform carries the layer k: the vertex
    is (clip x, clip y, w), and layer k lies in front of every lower one (reversed Z)"""
    vp = np.zeros((4, 4), dtype=f32)  # [column][row]
    vp[0][0] = vp[1][1] = 1
    vp[2][2] = 0.45
    vp[3][2] = 0.1
    vp[2][3] = 1
    return A.scene_struct(SC.IDENT, SC.IDENT, vp, [0.1] * 4, (0.2, 1, 0.5, 1), (1, 1, 1, 1))


def layer_transform(k):
    t = GL.identity().copy()
    t[2][3] = k  # the transformed vertex's fourth component is k z instead of 1
    t[3][3] = 0
    return t


EXPECTED = None  # a list while expected_sides() records: (label, corners, the predicate's intended answer)


def tri(corners, want=None, label=""):
    """corners: three of (px, py, w, u, v) -> (positions, uvs); want: the side of the predicate the triangle is meant for"""
    if EXPECTED is not None and want is not None:
        EXPECTED.append((label, list(corners), want))
    pos, uv = [], []
    for px, py, w, u, v in corners:
        x, y = clip_xy(px, py)
        pos.append((f32(x) * f32(w), f32(y) * f32(w), f32(w)))
        uv.append((u, v))
    return pos, uv


def quad(x0, y0, x1, y1, w, uvs=None, want=None, label=""):
    """two triangles over [x0, x1] x [y0, y1]; w and uv per corner"""
    w = w if isinstance(w, (list, tuple)) else [w] * 4
    uvs = uvs or [(0.0, 0.0), (1.5, 0.0), (1.5, 1.0), (0.0, 1.0)]
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    v = [(c[k][0], c[k][1], w[k], uvs[k][0], uvs[k][1]) for k in range(4)]
    return [tri([v[0], v[1], v[2]], want, label), tri([v[0], v[2], v[3]], want, label)]


def ranges_frame(r):
    SUB = 1.0 / 256.0
    img = r.create_image(S.make_texture(np.random.default_rng(29), 64, 0), mipmapped=True)
    smp = r.create_sampler(**S.SAMPLER_TRILINEAR)
    mo = r.write_material(A.PASS_MAIN_COLOR, (0.9, 0.8, 1.0, 1), img, smp)
    mt = r.write_material(A.PASS_TRANSPARENT, (0.3, 0.3, 0.2, 1), img, smp)
    layers = {0: [], 1: []}
    pixels = []
    layers[0] += quad(0, 0, W, H, [1.0, 2.0, 3.0, 2.0], [(0, 0), (6, 0), (6, 4), (0, 4)], True, "background")  # the common background
    # slivers along a row and a column of pixel centres, the third corner's depth off by delta
    for n, delta in enumerate((1.0 / 2048.0, 1.0 / 32.0, 0.5)):
        y = 10.5 + 6 * n
        layers[1].append(tri([(10.0, y, 1.0, 0.0, 0.0), (150.0, y - SUB, 2.0, 3.0, 0.2), (150.0, y + SUB, 2.0 * (1.0 + delta), 3.0, 0.3)],
                             delta < 0.001, f"row sliver, delta {delta}"))
        x = 12.5 + 6 * n
        layers[1].append(tri([(x, 30.0, 1.5, 0.0, 0.0), (x - SUB, 94.0, 1.0, 0.2, 2.0), (x + SUB, 94.0, 1.0 / (1.0 + delta), 0.3, 2.0)],
                             delta < 0.001, f"column sliver, delta {delta}"))
        pixels += [(80, int(y)), (int(x), 60)]
    # planes 1/w = gain (x - xh) whose far corners lie d pixels from the horizon x = xh
    xh, gain = 30.0, 0.01
    for n, d in enumerate((1.6, 1.05, 0.6, 0.05)):
        y = 30.0 + 9.0 * n
        c = [(xh + d, y), (xh + d, y + 8.0), (xh + 70.0, y + 4.0)]
        layers[1].append(tri([(px, py, 1.0 / (gain * (px - xh)), 0.02 * px, 0.05 * py) for px, py in c], d > 1.0, f"grazing, {d} px"))
        pixels.append((int(xh + d) + 2, int(y) + 4))
    # w scaled by powers of two, to the ends of the reciprocal's window and past them
    for n, s in enumerate((40, -40, 70, -70, 93, -93, 96, -97)):
        x0, y0 = 104 + 14 * (n % 4), 28 + 12 * (n // 4)
        layers[1] += quad(x0, y0, x0 + 13, y0 + 11, [float(np.ldexp(v, s)) for v in (1.0, 1.25, 1.5, 1.25)], None, abs(s) <= 93, f"w scaled by 2^{s}")
        pixels.append((x0 + 6, y0 + 5))
    # u at the guard's limit, past it, and not finite
    for n, u in enumerate((4194303.0, 1048576.0, 4194304.0, 8388608.0, np.inf, np.nan)):
        x0, y0 = 104 + 9 * n, 54
        layers[1] += quad(x0, y0, x0 + 8, y0 + 10, [1.0, 1.5, 2.0, 1.5], [(u, 0.0), (1.5, 0.0), (1.5, 1.0), (0.0, -u if n % 2 else 1.0)], n == 1, f"u = {u}")
        pixels.append((x0 + 4, y0 + 5))
    # a grazing triangle that reaches beyond the guard band: the clipper's pieces decide for themselves
    c = [(xh + 30.0, 68.0), (xh + 0.6, 80.0), (xh + 40000.0, 92.0)]
    layers[1].append(tri([(px, py, 1.0 / (1.0e-3 * (px - xh)), 0.02 * min(px, 500.0), 0.05 * py) for px, py in c]))
    pixels += [(40, 78), (100, 74)]
    opaque = []
    for k, tris in layers.items():
        pos = np.concatenate([np.asarray(p, dtype=f32) for p, _ in tris])
        uv = np.concatenate([np.asarray(t, dtype=f32) for _, t in tris])
        n = len(pos)
        verts = SC.make_vertices(pos, [(0.2, 0.9, 0.4)] * n, uv, [(0.8, 0.9, 1.0, 1)] * n)
        mesh = r.upload_mesh(np.arange(n, dtype=np.uint32), verts)
        opaque.append(SC.render_object(mesh, mo, 0, n, transform=layer_transform(k), **BOUNDS))
    # ordered pass: common, demoted (u = 2^22 at a corner), common, one over the other
    transparent = []
    for n, u in enumerate((1.0, 4194304.0, 2.0)):
        tris = quad(60 + 3 * n, 66 + 2 * n, 100 + 3 * n, 90 + 2 * n, [1.0, 1.2, 1.4, 1.2], [(u, 0.0), (1.5, 0.0), (1.5, 1.0), (0.0, 1.0)], u < 4.0, f"transparent, u = {u}")
        pos = np.concatenate([np.asarray(p, dtype=f32) for p, _ in tris])
        uv = np.concatenate([np.asarray(t, dtype=f32) for _, t in tris])
        mesh = r.upload_mesh(np.arange(6, dtype=np.uint32), SC.make_vertices(pos, [(0, 1, 0)] * 6, uv, [(0.5, 0.4, 0.3, 1)] * 6))
        transparent.append(SC.render_object(mesh, mt, 0, 6, transform=layer_transform(2), **BOUNDS))
    pixels.append((80, 78))
    return projective_scene(), SC.objs(opaque), SC.objs(transparent), pixels


FRAMES = {"textures": textures_frame, "ranges": ranges_frame}


# ---------------------------------------------------------------------------------------------- the intended sides
class _NoRenderer:
    """takes ranges_frame's uploads and hands out nothing: only the triangles are wanted"""

    def __getattr__(self, name):
        return lambda *a, **k: 0


def expected_sides():
    global EXPECTED
    EXPECTED = []
    try:
        ranges_frame(_NoRenderer())
        return EXPECTED
    finally:
        EXPECTED = None


def record_line(corners):
    """The record fields frag_ranges_ok reads, as setup_triangle forms them from the three corners (csrc/svr_device.h: C3
    viewport, C4 snap, orientation, edge steps, fp32 planes), one line for tests/native/frag_predicate_cli.cpp."""
    X, Y, rw, uv = [], [], [], []
    for px, py, w, u, v in corners:
        x, y = clip_xy(px, py)
        w = f32(w)
        r = f32(1) / w
        X.append(int(np.rint(f32(f32(f32(f32(x) * w) * r) * f32(W / 2) + f32(W / 2)) * f32(256))))
        Y.append(int(np.rint(f32(f32(f32(f32(y) * w) * r) * f32(H / 2) + f32(H / 2)) * f32(256))))
        rw.append(r)
        uv += [f32(u), f32(v)]
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    assert area2 != 0
    if area2 < 0:
        for a in (X, Y, rw):
            a[1], a[2] = a[2], a[1]
        area2 = -area2
    edge = lambda a, b: (-(Y[b] - Y[a]) * 256, (X[b] - X[a]) * 256)  # (A, B) of the edge from corner a to corner b
    (a1, b1), (a2, b2) = edge(2, 0), edge(0, 1)
    inv = f32(1) / f32(area2)
    hexbits = lambda f: format(int(np.array(f, dtype=f32).view(np.uint32)), "x")
    words = [hexbits(rw[0]), hexbits(f32(rw[1] - rw[0])), hexbits(f32(rw[2] - rw[0])), str(a1), str(b1), str(a2), str(b2), hexbits(inv)]
    return " ".join(words + [hexbits(t) for t in uv])


def test_triangles_fall_on_their_sides(tmp_path):
    import test_frag_setup as host
    (tmp_path / "frag_setup_under_test.h").write_text(host.setup_helpers())
    exe = str(tmp_path / "frag_predicate_cli")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", str(tmp_path), "-o", exe,
                    os.path.join(g.ROOT, "tests", "native", "frag_predicate_cli.cpp")], check=True)
    cases = expected_sides()
    with np.errstate(all="ignore"):
        text = "\n".join(record_line(c) for _, c, _ in cases) + "\n"
    got = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert len(got) == len(cases)
    wrong = [(label, want) for (label, _, want), ans in zip(cases, got) if bool(int(ans)) != bool(want)]
    assert not wrong, f"(triangle, intended answer) the predicate answers otherwise: {wrong}"
    sides = {bool(want) for _, _, want in cases}
    assert sides == {True, False} and len(cases) > 40


# ---------------------------------------------------------------------------------------------- rendering
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def plain(lib, frame, fmt, instrumented, traced):
    """the frame through svr_draw_geometry; traced: one more instrumented pass per traced pixel, its 64 trace slots"""
    r = lib.create(W, H, fmt)
    scene, opaque, transparent, pixels = FRAMES[frame](r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
    r.clear_color((0.25, 0.5, 0.75, 1))
    r.draw_geometry(scene, opaque, transparent)
    out = T._finish(r)
    out["pixels"], out["traces"] = pixels, []
    if traced:
        r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
        for x, y in pixels:
            r.trace_pixel(x, y)
            r.clear_color((0.25, 0.5, 0.75, 1))
            r.draw_geometry(scene, opaque, transparent)
            r.sync()
            out["traces"].append(r.read_trace().copy())
    r.close()
    return out


_ORACLE = {}


def reference(oracle, frame, fmt):
    if (frame, fmt) not in _ORACLE:
        _ORACLE[(frame, fmt)] = plain(oracle, frame, fmt, 1, True)
    return _ORACLE[(frame, fmt)]


def assert_frame(got, ref, what):
    for key in ("color", "depth"):
        T.assert_images_identical(got[key], ref[key], f"{what} {key}")


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_plain_passes_and_traces(hip, oracle, frame, fmt, instrumented):
    ref = reference(oracle, frame, FORMATS[fmt])
    assert ref["stats"].triangle_count > 40 and len(np.unique(ref["color"].reshape(-1, 4), axis=0)) > W * H // 8, "the frame is drawn at all"
    got = plain(hip, frame, FORMATS[fmt], instrumented, bool(instrumented))
    assert_frame(got, ref, f"{frame} {fmt}")
    hit = 0
    for (x, y), a, b in zip(ref["pixels"], got["traces"], ref["traces"]):
        a, b = a[TRACE_SLOTS], b[TRACE_SLOTS]
        differ = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))  # (a NaN's sign and payload are the machine's, not the contract's)
        assert not differ.any(), f"{frame} {fmt}: trace of pixel ({x}, {y}): slots {TRACE_SLOTS[differ].tolist()} differ"
        hit += int(b[0] != 0.0)
    if instrumented:
        assert hit >= len(ref["pixels"]) * 3 // 4, "the traced pixels lie on the cases"


@pytest.mark.parametrize("instrumented", [0, 1], ids=["timed", "instrumented"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_instance(hip, oracle, frame, fmt, instrumented):
    """the ID, multiview, attribute, depth-load and draw-list instances: their colour and depth are the plain pass's"""
    torch = pytest.importorskip("torch")
    ref = reference(oracle, frame, FORMATS[fmt])
    clear = (0.25, 0.5, 0.75, 1)
    r = hip.create(W, H, FORMATS[fmt])
    scene, opaque, transparent, _ = FRAMES[frame](r)
    r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)

    def check(what):
        assert_frame(T._finish(r), ref, f"{frame} {fmt} {what}")

    lst = r.create_draw_list(opaque, transparent)
    r.clear_color(clear)
    r.draw_list(scene, lst)
    check("draw list")

    r.enable_ids()
    r.clear_color(clear)
    r.draw_geometry(scene, opaque, transparent)
    check("ID target")
    ids = r.read_ids()
    assert len(np.unique(ids[..., 0])) >= 2 and ids[..., 1].max() > 0
    r.enable_ids(False)

    r.enable_attributes(A.ATTR_ALL)
    r.clear_color(clear)
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
    r.clear_color(clear)
    r.draw_geometry(scene, opaque, transparent)
    check("depth load")
    r.set_depth_load_op(A.DEPTH_CLEAR)
    r.bind_targets(None, None)

    # two views of the same scene: both layers are the frame
    layers = torch.zeros((2, H, W, 4), dtype=cdt, device="cuda")
    depths = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for how in ("geometry", "list"):
        if how == "geometry":
            r.draw_views([scene, scene], layers.data_ptr(), depths.data_ptr(), opaque, transparent, clear_rgba=clear)
        else:
            r.draw_list_views([scene, scene], lst, layers.data_ptr(), depths.data_ptr(), clear_rgba=clear)
        r.sync()
        torch.cuda.synchronize()
        c = layers.cpu().numpy().view(np.uint16 if FORMATS[fmt] == A.COLOR_RGBA16F else np.uint8)
        d = depths.cpu().numpy()
        for k in range(2):
            T.assert_images_identical(c[k], ref["color"], f"{frame} {fmt} views ({how}) layer {k} color")
            T.assert_images_identical(d[k], ref["depth"], f"{frame} {fmt} views ({how}) layer {k} depth")
    lst.close()
    r.close()
