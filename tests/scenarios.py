"""Small hand-built scenes rendered through the svr.h ABI.  Each scenario takes a library (oracle or
HIP) and returns {"color": fp16 bits [H,W,4], "depth": f32 [H,W], "rgba8", "stats"}.  The oracle KATs
assert analytic properties of these; the GPU parity tests assert HIP == oracle bit for bit."""
import numpy as np

import __graft_entry__ as g
import svr_testlib as T

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
f32 = np.float32
IDENT = GL.identity()


def identity_scene(ambient=0.1, sun=(0, 1, 0.5, 1), sun_color=(1, 1, 1, 1)):
    """GPUSceneData with viewproj = I: vertex positions are clip coordinates."""
    return A.scene_struct(IDENT, IDENT, IDENT, [ambient] * 4, sun, sun_color)


def make_vertices(positions, normals=None, uvs=None, colors=None):
    n = len(positions)
    v = np.zeros(n, dtype=A.VERTEX_DTYPE)
    v["position"] = np.asarray(positions, dtype=f32)
    v["normal"] = np.asarray(normals, dtype=f32) if normals is not None else np.array([0, 1, 0], dtype=f32)
    v["color"] = np.asarray(colors, dtype=f32) if colors is not None else f32(1)
    if uvs is not None:
        uvs = np.asarray(uvs, dtype=f32)
        v["uv_x"], v["uv_y"] = uvs[:, 0], uvs[:, 1]
    return v


def render_object(mesh, material, first_index, index_count, transform=None, origin=(0, 0, 0), extents=(1, 1, 1)):
    ro = np.zeros((), dtype=A.RENDER_OBJECT_DTYPE)
    ro["index_count"], ro["first_index"], ro["mesh"], ro["material"] = index_count, first_index, mesh, material
    ro["origin"], ro["extents"] = origin, extents
    ro["sphere_radius"] = float(np.linalg.norm(np.asarray(extents, dtype=np.float64)))
    ro["transform"] = (IDENT if transform is None else transform).reshape(16)
    return ro


def objs(lst):
    return np.array(lst, dtype=A.RENDER_OBJECT_DTYPE) if lst else np.zeros(0, dtype=A.RENDER_OBJECT_DTYPE)


class Rig:
    """A context with the engine's default resources (src/vk_engine.cpp:226-283)."""

    def __init__(self, lib, w, h, color_format=A.COLOR_RGBA16F, background=(1, 1, 1, 1)):
        self.r = lib.create(w, h, color_format)
        self.r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
        self.white = self.r.create_image(S.white_1x1())
        self.checker = self.r.create_image(S.checkerboard_32())
        self.nearest = self.r.create_sampler(**S.SAMPLER_NEAREST)
        self.linear = self.r.create_sampler(**S.SAMPLER_LINEAR)
        self.trilinear = self.r.create_sampler(**S.SAMPLER_TRILINEAR)
        self.background = background

    def material(self, color=(1, 1, 1, 1), image=None, sampler=None, transparent=False):
        return self.r.write_material(A.PASS_TRANSPARENT if transparent else A.PASS_MAIN_COLOR, color,
                                     image if image is not None else self.white,
                                     sampler if sampler is not None else self.linear)

    def draw(self, scene, opaque, transparent=()):
        self.r.clear_color(self.background)
        st = self.r.draw_geometry(scene, objs(list(opaque)), objs(list(transparent)))
        return st

    def finish(self):
        out = T._finish(self.r)
        self.r.close()
        return out


QUAD_IDX = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)


def clip_quad(x0, y0, x1, y1, z, normal=(0, 1, 0), color=(1, 1, 1, 1), uv_scale=1.0):
    """Axis-aligned quad in clip space (w = 1), two triangles sharing the (x0,y0)-(x1,y1) diagonal."""
    pos = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    uv = [(0, 0), (uv_scale, 0), (uv_scale, uv_scale), (0, uv_scale)]
    return make_vertices(pos, [normal] * 4, uv, [color] * 4)


# ----------------------------------------------------------------------------------------------
def shading_constants(lib, normal, size=32):
    """Full-screen quad, 1x1 white texture, vertex colour 1, given normal (SURVEY.md §8c goldens)."""
    rig = Rig(lib, size, size)
    mesh = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 1, 0.5, normal=normal))
    mat = rig.material()
    rig.draw(identity_scene(), [render_object(mesh, mat, 0, 6)])
    return rig.finish()


def shared_edge_additive(lib, size=64):
    """Two triangles sharing a diagonal, additive-blended over black: a double hit would show as 2x,
    a hole as 0 (top-left rule)."""
    rig = Rig(lib, size, size, background=(0, 0, 0, 1))
    mesh = rig.r.upload_mesh(QUAD_IDX, clip_quad(-0.83, -0.71, 0.77, 0.9, 0.5, normal=(0, 1, 0)))
    mat = rig.material(transparent=True)
    rig.draw(identity_scene(), [], [render_object(mesh, mat, 0, 6)])
    return rig.finish()


def fan_additive(lib, size=96, n=23):
    """A fan of thin triangles around an off-centre vertex, additive over black: every interior
    pixel must be hit exactly once whatever the slopes."""
    rig = Rig(lib, size, size, background=(0, 0, 0, 1))
    ang = np.linspace(0, 2 * np.pi, n + 1)
    ring = np.stack([0.93 * np.cos(ang), 0.88 * np.sin(ang), np.full_like(ang, 0.5)], axis=1)
    pos = np.concatenate([[(0.1173, -0.0631, 0.5)], ring])
    idx = np.array([[0, 1 + i, 2 + i] for i in range(n)], dtype=np.uint32).reshape(-1)
    mesh = rig.r.upload_mesh(idx, make_vertices(pos))
    mat = rig.material(transparent=True)
    rig.draw(identity_scene(), [], [render_object(mesh, mat, 0, idx.size)])
    return rig.finish()


def depth_order(lib, later_is_nearer, size=32):
    """Two overlapping quads at different depths (reversed-Z: larger = nearer), red then green."""
    rig = Rig(lib, size, size)
    za, zb = (0.25, 0.75) if later_is_nearer else (0.75, 0.25)
    ma = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 0.5, 0.5, za, color=(1, 0, 0, 1)))
    mb = rig.r.upload_mesh(QUAD_IDX, clip_quad(-0.5, -0.5, 1, 1, zb, color=(0, 1, 0, 1)))
    mat = rig.material()
    rig.draw(identity_scene(), [render_object(ma, mat, 0, 6), render_object(mb, mat, 0, 6)])
    return rig.finish()


def depth_tie(lib, size=32):
    """Coplanar identical quads, red then green with the same material: GREATER_OR_EQUAL lets the
    later draw win (src/vk_engine.cpp:1659)."""
    rig = Rig(lib, size, size)
    ma = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 1, 0.5, color=(1, 0, 0, 1)))
    mb = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 1, 0.5, color=(0, 1, 0, 1)))
    mat = rig.material()
    rig.draw(identity_scene(), [render_object(ma, mat, 0, 6), render_object(mb, mat, 0, 6)])
    return rig.finish()


def transparent_layers(lib, size=32):
    """Opaque grey quad at z=0.5 on the left half; three transparent quads: in front (z=.6) over
    everything, behind the opaque one (z=.4) and a second in-front layer.  No depth write."""
    rig = Rig(lib, size, size, background=(0.25, 0.25, 0.25, 1))
    op = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 0, 1, 0.5, color=(0.5, 0.5, 0.5, 1)))
    t1 = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 0, 0.6, color=(0.3, 0.0, 0.0, 1)))
    t2 = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 1, 0.4, color=(0.0, 0.2, 0.0, 1)))
    t3 = rig.r.upload_mesh(QUAD_IDX, clip_quad(-0.5, -1, 0.5, 1, 0.7, color=(0.0, 0.0, 0.1, 1)))
    mo, mt = rig.material(), rig.material(transparent=True)
    rig.draw(identity_scene(ambient=0.0, sun=(0, 1, 0, 1)),
             [render_object(op, mo, 0, 6)],
             [render_object(t1, mt, 0, 6), render_object(t2, mt, 0, 6), render_object(t3, mt, 0, 6)])
    return rig.finish()


def textured_plane(lib, sampler_kind, size=64, tiles=23.5, mip=True):
    """A quad with the 32x32 checker repeated `tiles` times: heavy minification."""
    rig = Rig(lib, size, size)
    img = rig.r.create_image(S.checkerboard_32(), mipmapped=mip)
    smp = {"nearest": rig.nearest, "linear": rig.linear, "trilinear": rig.trilinear}[sampler_kind]
    mesh = rig.r.upload_mesh(QUAD_IDX, clip_quad(-1, -1, 1, 1, 0.5, uv_scale=tiles))
    mat = rig.material(image=img, sampler=smp)
    rig.draw(identity_scene(ambient=0.0, sun=(0, 1, 0, 1)), [render_object(mesh, mat, 0, 6)])
    return rig.finish()


def perspective_floor(lib, w=96, h=64, sampler_kind="trilinear"):
    """A ground plane under a real camera: perspective-correct uv, anisotropic minification, the far
    end clipped by z>=0 and the near end by z<=w (it extends behind the camera)."""
    rig = Rig(lib, w, h)
    img = rig.r.create_image(S.checkerboard_32(), mipmapped=True)
    smp = {"nearest": rig.nearest, "linear": rig.linear, "trilinear": rig.trilinear}[sampler_kind]
    L = 3.0e4
    pos = [(-L, 0, -L), (L, 0, -L), (L, 0, L), (-L, 0, L)]
    uv = [(0, 0), (L, 0), (L, L), (0, L)]
    mesh = rig.r.upload_mesh(QUAD_IDX, make_vertices(pos, [(0, 1, 0)] * 4, uv))
    mat = rig.material(image=img, sampler=smp)
    scene = S.scene_data_struct((0.0, 1.5, 0.0), 0.0, 0.3, w, h)
    # bounds are caller data: with the true extents every corner is beyond the far plane or behind
    # the eye and is_visible (no w guard, z-range test) culls the floor although it fills the view —
    # the reference's behaviour, covered by test_is_visible.  Hand in bounds that pass.
    rig.draw(scene, [render_object(mesh, mat, 0, 6, extents=(1000, 0, 1000))])
    return rig.finish()


def near_clip_wall(lib, w=80, h=60):
    """A wall the camera nearly touches and that crosses the near plane and the guard band."""
    rig = Rig(lib, w, h)
    img = rig.r.create_image(S.checkerboard_32(), mipmapped=True)
    pos = [(-50, -40, -3.0), (60, -40, 1.0), (60, 45, 1.0), (-50, 45, -3.0)]
    uv = [(0, 0), (9, 0), (9, 7), (0, 7)]
    mesh = rig.r.upload_mesh(QUAD_IDX, make_vertices(pos, [(0.3, 0.5, 1)] * 4, uv))
    mat = rig.material(image=img, sampler=rig.trilinear)
    scene = S.scene_data_struct((0.0, 0.0, 0.0), 0.1, -0.2, w, h)
    # true bounds would be culled by is_visible's missing w<=0 guard (box straddles the eye plane)
    rig.draw(scene, [render_object(mesh, mat, 0, 6, origin=(0, 0, -5), extents=(1, 1, 1))])
    return rig.finish()


def depth_plane(lib, distance, size=16):
    """Camera at the origin looking down -z at a big quad `distance` away."""
    rig = Rig(lib, size, size)
    e = distance * 4.0
    pos = [(-e, -e, -distance), (e, -e, -distance), (e, e, -distance), (-e, e, -distance)]
    mesh = rig.r.upload_mesh(QUAD_IDX, make_vertices(pos))
    mat = rig.material()
    scene = S.scene_data_struct((0.0, 0.0, 0.0), 0.0, 0.0, size, size)
    rig.draw(scene, [render_object(mesh, mat, 0, 6, extents=(e, e, 0), origin=(0, 0, -distance))])
    return rig.finish()


def random_soup(lib, w=160, h=96, n_tris=600, seed=7, transparent_every=5, color_format=A.COLOR_RGBA16F,
                scissor=None, big=3):
    """Seeded triangle soup in clip space with w != 1, all sizes incl. sub-pixel and screen-filling,
    some beyond the guard band, mixed opaque/transparent, textured."""
    rng = np.random.default_rng(seed)
    rig = Rig(lib, w, h, color_format)
    img = rig.r.create_image(S.make_texture(np.random.default_rng(seed + 1), 64, 0), mipmapped=True)
    n = n_tris
    centre = rng.uniform(-1.1, 1.1, (n, 1, 2))
    scale = 10.0 ** rng.uniform(-2.5, -0.3, (n, 1, 1))
    scale[:big] = 3.0
    scale[big:2 * big] = 4.0e3  # far outside the guard band: goes through the clipper
    xy = centre + rng.normal(0, 1, (n, 3, 2)) * scale
    wv = rng.uniform(0.6, 2.5, (n, 3, 1))
    wv[-8:] = rng.uniform(-0.5, 1.0, (8, 3, 1))  # some vertices behind the eye
    z = rng.uniform(0.02, 0.98, (n, 3, 1)) * wv
    pos_clip = np.concatenate([xy * wv, z, wv], axis=2).reshape(-1, 4)
    # positions must be vec3: fold w into the world matrix per triangle is not possible, so use a
    # projective viewproj instead: clip = M * (x,y,z,1) with M's last row (0,0,1,0) -> w = z_in
    pos3 = np.stack([pos_clip[:, 0], pos_clip[:, 1], pos_clip[:, 3]], axis=1)  # z_in = w
    vp = np.zeros((4, 4), dtype=f32)
    vp[0][0] = vp[1][1] = 1
    vp[2][2] = 0.45   # clip.z = 0.45*w + 0.1  (inside [0,w] for w in (0.19, ..))
    vp[3][2] = 0.1
    vp[2][3] = 1      # clip.w = z_in
    verts = make_vertices(pos3, rng.normal(0, 1, (3 * n, 3)), rng.uniform(-2, 3, (3 * n, 2)),
                          np.concatenate([rng.uniform(0.2, 1, (3 * n, 3)), np.ones((3 * n, 1))], axis=1))
    idx = np.arange(3 * n, dtype=np.uint32)
    mesh = rig.r.upload_mesh(idx, verts)
    mo = rig.material(color=(0.9, 0.8, 1.0, 1), image=img, sampler=rig.trilinear)
    mt = rig.material(color=(0.3, 0.3, 0.2, 1), image=img, sampler=rig.linear, transparent=True)
    opaque, transparent = [], []
    for t in range(n):
        ro = render_object(mesh, mt if (transparent_every and t % transparent_every == 0) else mo, 3 * t, 3,
                           extents=(1e6, 1e6, 1e6))
        (transparent if (transparent_every and t % transparent_every == 0) else opaque).append(ro)
    scene = A.scene_struct(IDENT, IDENT, vp, [0.1] * 4, (0.2, 1, 0.5, 1), (1, 1, 1, 1))
    if scissor:
        rig.r.set_scissor(*scissor)
    rig.draw(scene, opaque, transparent)
    return rig.finish()


def transparent_stack(lib, n_layers, size=48, jitter=0.0, seed=21):
    """n_layers small transparent quads stacked on the same pixels (one 32x32 tile holds 2*n_layers
    triangles): deep in-order blending.  More than 1024 layers exceeds the tile kernel's LDS sort
    capacity (2048 entries) and sorts in the global arena."""
    rng = np.random.default_rng(seed)
    rig = Rig(lib, size, size, background=(0.0, 0.0, 0.0, 1))
    verts, idx = [], []
    for i in range(n_layers):
        cx, cy = rng.uniform(-jitter, jitter, 2)
        x0, y0 = -0.62 + cx, -0.55 + cy
        c = (0.004 + 0.003 * (i % 5), 0.002 * (i % 3), 0.001 * (i % 7), 1)
        verts.append(clip_quad(x0, y0, x0 + 0.5, y0 + 0.45, 0.3 + 0.4 * (i % 11) / 11.0, color=c))
        idx.append(QUAD_IDX + 4 * i)
    back = clip_quad(-1, -1, 0.1, 1, 0.5, color=(0.2, 0.2, 0.2, 1))  # opaque: hides the layers behind z=.5 on the left
    mesh = rig.r.upload_mesh(np.concatenate(idx), np.concatenate(verts))
    mb = rig.r.upload_mesh(QUAD_IDX, back)
    mo, mt = rig.material(), rig.material(transparent=True)
    rig.draw(identity_scene(ambient=0.0, sun=(0, 1, 0, 1)), [render_object(mb, mo, 0, 6)],
             [render_object(mesh, mt, 0, 6 * n_layers)])
    return rig.finish()


def transparent_stack_clipped(lib, n_layers=120, size=48):
    """Transparent quads that cross the z = w plane: the clipper cuts every triangle into a fan of pieces with
    the parent's submission key, and tiles on the cut hold several pieces of one triangle — equal sort keys
    in one (split) tile's transparent bin."""
    rig = Rig(lib, size, size, background=(0.0, 0.0, 0.0, 1))
    verts, idx = [], []
    for i in range(n_layers):
        zl, zr = 0.15 + 0.004 * (i % 9), 1.5 + 0.01 * (i % 7)  # left edge inside, right edge beyond the plane
        y0 = -0.9 + 0.002 * (i % 5)
        c = (0.004 + 0.003 * (i % 5), 0.002 * (i % 3), 0.001 * (i % 7), 1)
        pos = [(-0.9, y0, zl), (0.9, y0, zr), (0.9, 0.9, zr), (-0.9, 0.9, zl)]
        verts.append(make_vertices(pos, [(0, 1, 0)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)], [c] * 4))
        idx.append(QUAD_IDX + 4 * i)
    mesh = rig.r.upload_mesh(np.concatenate(idx), np.concatenate(verts))
    mt = rig.material(transparent=True)
    rig.draw(identity_scene(ambient=0.0, sun=(0, 1, 0, 1)), [], [render_object(mesh, mt, 0, 6 * n_layers)])
    return rig.finish()


def ragged_draws(lib, size=48):
    """index_count not a multiple of 3, zero-length draws, an empty opaque list entry order."""
    rig = Rig(lib, size, size)
    v = np.concatenate([clip_quad(-1, -1, 0, 0, 0.5, color=(1, 0, 0, 1)), clip_quad(0, 0, 1, 1, 0.4, color=(0, 0, 1, 1))])
    idx = np.array([0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7], dtype=np.uint32)
    mesh = rig.r.upload_mesh(idx, v)
    mat = rig.material()
    rig.draw(identity_scene(), [render_object(mesh, mat, 0, 5), render_object(mesh, mat, 6, 0),
                                render_object(mesh, mat, 6, 6), render_object(mesh, mat, 3, 2)])
    return rig.finish()


def empty_frame(lib, size=40):
    rig = Rig(lib, size, size)
    rig.draw(identity_scene(), [], [])
    return rig.finish()


# ---------------------------------------------------------------------------------------------- hierarchical depth test
# Opaque scenes aimed at the tile kernel's hierarchical depth test (csrc/k_tile.hip: the occluder claim and the 8x8
# block minima of scan_columns, the deep-bin filter of tile_body).  That test only runs on bins of more than 64 opaque
# triangles, so every tile these scenes aim at gets more.  The geometry is given in pixels, (px, py, depth), and placed
# in clip space with w = 1: the viewport maps it back exactly (x_s = px, y_s = py, depth = z), so pixel centres,
# sub-pixel offsets and depths are what the numbers say.  Each layer is one mesh object.  hiz_geometry(name) returns a
# scene's layers without rendering it, for the CPU checks of what each scene reaches (tests/test_hiz_scenarios.py).
SUB = 1.0 / 256.0  # one step of the 24.8 snap (DESIGN C4)


class Layer:
    def __init__(self, tris, color):
        self.tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)  # (triangle, vertex, (px, py, z))
        self.color = color


class HizScene:
    def __init__(self, w, h, layers, scissor=None, color_format=A.COLOR_RGBA16F):
        self.w, self.h, self.layers, self.scissor, self.color_format = w, h, layers, scissor, color_format


def px_quad(x0, y0, x1, y1, z):
    """The rectangle [x0, x1] x [y0, y1] in pixels (edges on pixel boundaries cover whole pixels): two triangles."""
    return [[(x0, y0, z), (x1, y0, z), (x1, y1, z)], [(x0, y0, z), (x1, y1, z), (x0, y1, z)]]


def tile_occluder(tx, ty, z):
    """One triangle that covers tile (tx, ty) and reaches at most 31 pixels into the tiles right of and below it: its
    right angle one pixel above and left of the tile, legs 65.5 px.  Scenes with such occluders put their aimed tiles
    on even tile coordinates (SLOTS) and leave the odd ones to the overhang."""
    ox, oy = 32.0 * tx, 32.0 * ty
    return [(ox - 1, oy - 1, z), (ox + 64.5, oy - 1, z), (ox - 1, oy + 64.5, z)]


SLOTS = [(0, 0), (2, 0), (0, 2), (2, 2)]


def render_hiz(lib, sc):
    rig = Rig(lib, sc.w, sc.h, sc.color_format, background=(0, 0, 0, 1))
    mat = rig.material()
    ros = []
    for layer in sc.layers:
        t = layer.tris
        if not len(t):
            continue
        pos = np.empty((len(t) * 3, 3), dtype=f32)
        pos[:, 0] = (t[:, :, 0].reshape(-1) * 2.0 / sc.w - 1.0).astype(f32)
        pos[:, 1] = (t[:, :, 1].reshape(-1) * 2.0 / sc.h - 1.0).astype(f32)
        pos[:, 2] = t[:, :, 2].reshape(-1).astype(f32)  # (keeps -0.0)
        mesh = rig.r.upload_mesh(np.arange(len(pos), dtype=np.uint32), make_vertices(pos, colors=[layer.color] * len(pos)))
        ros.append(render_object(mesh, mat, 0, len(pos), extents=(1e6, 1e6, 1e6)))
    if sc.scissor:
        rig.r.set_scissor(*sc.scissor)
    rig.draw(identity_scene(), ros)
    return rig.finish()


def _padding(rng, tiles, per_tile, zlo, zhi, size=(0.6, 3.0)):
    """per_tile small triangles inside each 32x32 tile (tx, ty), depths in [zlo, zhi)."""
    tris = []
    for tx, ty in tiles:
        c = rng.uniform(0, 32, (per_tile, 1, 2)) + (32 * tx, 32 * ty)
        v = c + rng.uniform(-1, 1, (per_tile, 3, 2)) * rng.uniform(*size, (per_tile, 1, 1))
        v = np.clip(v, (32 * tx, 32 * ty), (32 * tx + 31.99, 32 * ty + 31.99))
        z = np.repeat(rng.uniform(zlo, zhi, (per_tile, 1, 1)), 3, axis=1)
        tris.append(np.concatenate([v, z], axis=2))
    return np.concatenate(tris)


RED, GREEN, BLUE, GREY = (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 1), (0.5, 0.5, 0.5, 1)

# hiz_occluder_edges: one slot per tile, tile rows 0, 2, 4, ... (the odd rows take what the occluders overhang).
# Slot (corner, offset, flip): one triangle covering its tile whose two legs run along the tile's first or last row and
# column — through the pixel centres (offset 0), one sub-pixel step outside them (+1: the row is covered, the claim can
# hold) or inside (-1: the row is not covered).  The right angle sits at the corner; the legs run 36 px along y and far
# along x, away from the corner, so the hypotenuse passes beyond the tile.  flip swaps the winding.
EDGE_SLOTS = [(corner, off, flip) for off in (0, 1, -1) for corner in ((0, 0), (1, 0), (0, 1), (1, 1))
              for flip in ((0, 1) if off == 0 else (off < 0,))]
EDGE_Z_FRONT, EDGE_Z_BACK, EDGE_Z_BACK2 = 0.75, 0.5, 0.375


def edge_slot_origin(k):
    # corner x = 1 (legs run left) goes in tile column 0, corner x = 0 (legs run right) in column 1: the far leg leaves
    # the frame without crossing the other column's slots
    corner = EDGE_SLOTS[k][0]
    return (0 if corner[0] else 32), 64 * _edge_row(k)


def _edge_row(k):
    col = 0 if EDGE_SLOTS[k][0][0] else 1
    return sum(1 for j in range(k) if (0 if EDGE_SLOTS[j][0][0] else 1) == col)


def hiz_occluder_edges_geometry(seed=31):
    rng = np.random.default_rng(seed)
    rows = max(_edge_row(k) for k in range(len(EDGE_SLOTS))) + 1
    w, h = 64, 64 * rows
    front, back, back2, tiles = [], [], [], []
    for k, ((cx, cy), off, flip) in enumerate(EDGE_SLOTS):
        ox, oy = edge_slot_origin(k)
        tiles.append((ox // 32, oy // 32))
        sx, sy = (1, -1)[cx], (1, -1)[cy]  # legs run away from the corner
        px = ox + (31.5 if cx else 0.5) - sx * off * SUB
        py = oy + (31.5 if cy else 0.5) - sy * off * SUB
        a, b, c = (px, py, EDGE_Z_FRONT), (px + sx * 4000.0, py, EDGE_Z_FRONT), (px, py + sy * 36.0, EDGE_Z_FRONT)
        front.append([a, c, b] if flip else [a, b, c])
        back += px_quad(ox, oy, ox + 32, oy + 32, EDGE_Z_BACK)
        back2 += px_quad(ox - 8, oy - 8, ox + 40, oy + 40, EDGE_Z_BACK2)  # larger, behind, drawn after
    pad = _padding(rng, tiles, 200, 0.05, 0.35)
    layers = [Layer(pad, GREY), Layer(back, BLUE), Layer(front, RED), Layer(back2, GREEN)]
    return HizScene(w, h, layers)


# hiz_depth_margins: one tile (SLOTS) per kind of front plane — constant, sloped, steep (|dz1|, |dz2| >> z0) and constant
# again under near-degenerate slivers.  The front is one triangle over its tile, drawn twice (the later copy, GREEN, must
# win every pixel: ties go to the later object).  Behind it come full-tile layers 64, 8, 2 and 1 ulps and about 2^-21
# relative below the front's smallest pixel depth in the tile, and last a layer AT it (BLUE: wins where it ties).
MARGIN_ULPS = (64, 8, 2, 1)
MARGIN_KINDS = ("constant", "sloped", "steep", "slivers")


def _front_plane(kind, ox, oy):
    """One triangle covering the tile at (ox, oy): (px, py, z) x 3 (tile_occluder)."""
    z = {"sloped": (0.55, 0.7, 0.6), "steep": (0.0009765625, 0.9990234375, 0.9990234375)}.get(kind, (0.625,) * 3)
    return [(x, y, zz) for (x, y, _), zz in zip(tile_occluder(ox // 32, oy // 32, 0.0), z)]


def _plane_min_depth(tri, ox, oy):
    """The smallest depth the rasteriser's float chain (DESIGN C5) gives the pixels of the tile: the oracle's setup in
    numpy (w = 1: vertices are snapped pixels, depths as given)."""
    X = np.rint(np.array([v[0] for v in tri]) * 256).astype(np.int64)
    Y = np.rint(np.array([v[1] for v in tri]) * 256).astype(np.int64)
    Z = np.array([v[2] for v in tri], dtype=f32)
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    if area2 < 0:
        X[[1, 2]], Y[[1, 2]], Z[[1, 2]], area2 = X[[2, 1]], Y[[2, 1]], Z[[2, 1]], -area2
    gy, gx = np.mgrid[oy:oy + 32, ox:ox + 32]
    PX, PY = gx.astype(np.int64) * 256 + 128, gy.astype(np.int64) * 256 + 128
    e = []
    for i in (1, 2):
        a, b = (i + 1) % 3, (i + 2) % 3
        e.append((X[b] - X[a]) * (PY - Y[a]) - (Y[b] - Y[a]) * (PX - X[a]))
    inv = f32(1.0) / f32(area2)
    b1, b2 = e[1].astype(f32) * inv, e[0].astype(f32) * inv  # edge 1 is opposite vertex 1: b1 (all inside: no bias)
    dz1, dz2 = f32(Z[1] - Z[0]), f32(Z[2] - Z[0])
    inner = (b1.astype(np.float64) * dz1 + Z[0]).astype(f32)  # fma: the product of two floats is exact in double
    z = (b2.astype(np.float64) * dz2 + inner).astype(f32)
    return f32(np.clip(z, 0, 1).min())


def hiz_depth_margins_geometry(seed=37):
    rng = np.random.default_rng(seed)
    fronts, zmins, tiles = [], [], []
    for k, kind in enumerate(MARGIN_KINDS):
        tx, ty = SLOTS[k]
        ox, oy = 32 * tx, 32 * ty
        tiles.append((tx, ty))
        tri = _front_plane(kind, ox, oy)
        fronts.append(tri)
        zmins.append(_plane_min_depth(tri, ox, oy))
    backs = {}
    for u in MARGIN_ULPS:
        backs[u] = sum((px_quad(32 * tx, 32 * ty, 32 * tx + 32, 32 * ty + 32,
                                float(np.nextafter(f32(zm), f32(0)) if u == 1 else f32(zm) - f32(u) * np.spacing(f32(zm))))
                        for (tx, ty), zm in zip(tiles, zmins)), [])
    rel = sum((px_quad(32 * tx, 32 * ty, 32 * tx + 32, 32 * ty + 32, float(f32(zm * (1.0 - 2.0 ** -21))))
               for (tx, ty), zm in zip(tiles, zmins)), [])
    tie = sum((px_quad(32 * tx, 32 * ty, 32 * tx + 32, 32 * ty + 32, float(zm)) for (tx, ty), zm in zip(tiles, zmins)), [])
    # slivers: areas of a few 1/256 px steps (inv_area in the thousands), across the last slot at the front's depth
    # and one ulp either side of it
    ox, oy = 32 * SLOTS[3][0], 32 * SLOTS[3][1]
    zf = f32(0.625)
    slivers = []
    for j in range(24):
        y = oy + 1.5 + j - SUB * (1 + j % 2)  # just above a row of pixel centres: the sliver crosses it
        zz = float([np.nextafter(zf, f32(0)), zf, np.nextafter(zf, f32(1))][j % 3])
        slivers.append([(ox - 28.0, y, zz), (ox + 3000.0, y + SUB * (1 + j % 4), zz), (ox + 17.0, y + SUB * (2 + j % 3), zz)])
    pad = _padding(rng, tiles, 200, 0.005, 0.04)  # behind every front, the steep one included
    layers = [Layer(pad, GREY), Layer(fronts, RED), Layer(fronts, GREEN)]
    layers += [Layer(backs[u], GREY) for u in MARGIN_ULPS] + [Layer(rel, GREY), Layer(slivers, (1, 1, 0, 1)), Layer(tie, BLUE)]
    return HizScene(96, 96, layers)


# hiz_deep_opaque_N: N opaque layers of two triangles over each of four tiles (one object per layer: each tile's bin
# holds 2 N triangles).  Depths come from a short list (repeats), in random order; a layer covers a tile whole, a run
# of its 8x8 blocks, or an arbitrary sub-pixel rectangle.  The nearest layer of each tile (FRONT_Z, full cover) lands
# late in tile 0 (a later filter window than most of what it hides), early in tile 1, twice in tile 2 (the later copy
# wins) and in tile 3 covers only half the tile's blocks.
DEEP_FRONT_Z = 0.875


def hiz_deep_opaque_geometry(n_layers, w=64, h=64, seed=41, scissor=None):
    rng = np.random.default_rng(seed + n_layers)
    levels = np.round(rng.uniform(0.1, 0.8, 24), 3)
    tiles = [(0, 0), (1, 0), (0, 1), (1, 1)]
    front_at = {0: [int(n_layers * 0.8)], 1: [3], 2: [2, n_layers - 2], 3: [n_layers // 2]}
    layers = []
    for i in range(n_layers):
        tris = []
        for t, (tx, ty) in enumerate(tiles):
            ox, oy = 32 * tx, 32 * ty
            if i in front_at[t]:
                if t == 3:
                    tris += px_quad(ox, oy, ox + 16, oy + 32, DEEP_FRONT_Z)
                else:
                    tris += px_quad(ox, oy, ox + 32, oy + 32, DEEP_FRONT_Z)
                continue
            z = float(rng.choice(levels))
            kind = rng.integers(0, 10)
            if kind < 6:
                tris += px_quad(ox, oy, ox + 32, oy + 32, z)
            elif kind < 8:
                bx0, by0 = rng.integers(0, 4, 2)
                bx1, by1 = bx0 + rng.integers(1, 5 - bx0), by0 + rng.integers(1, 5 - by0)
                tris += px_quad(ox + 8 * bx0, oy + 8 * by0, ox + 8 * bx1, oy + 8 * by1, z)
            else:
                x0, y0 = rng.uniform(0, 24, 2)
                tris += px_quad(ox + x0, oy + y0, ox + x0 + rng.uniform(1, 32 - x0), oy + y0 + rng.uniform(1, 32 - y0), z)
        c = (0.2 + 0.8 * ((i * 37) % 101) / 100.0, 0.2 + 0.8 * ((i * 53) % 97) / 96.0, 0.2 + 0.8 * ((i * 71) % 89) / 88.0, 1)
        layers.append(Layer(tris, c))
    return HizScene(w, h, layers, scissor=scissor)


# hiz_clipped_occluders: tile-covering occluders (SLOTS) that the clipper cuts (DESIGN C2), in front of 600-deep opaque
# stacks: slot 0's reaches beyond the guard band (x = -40 000 px), slot 1's crosses the near plane (z > w) below its
# tile, slot 2's does both, and in slot 3 the near plane cuts through the tile itself (what lies beyond it is not
# drawn: the stack shows there).
def hiz_clipped_occluders_geometry(seed=43, n_stack=600):
    rng = np.random.default_rng(seed)
    occ = [
        [(-40000.0, -1.0, 0.8), (64.5, -1.0, 0.8), (-1.0, 64.5, 0.8)],
        [(63.0, -1.0, 0.8), (128.5, -1.0, 0.8), (63.0, 64.5, 1.15)],
        [(-40000.0, 63.0, 0.8), (64.5, 63.0, 0.8), (-1.0, 128.5, 1.15)],
        [(63.0, 63.0, 0.8), (128.5, 63.0, 1.4), (63.0, 128.5, 0.8)],
    ]
    stack = []
    for i in range(n_stack):
        z = float(np.round(rng.uniform(0.1, 0.75), 2))
        stack.append(Layer(sum((px_quad(32 * tx, 32 * ty, 32 * tx + 32, 32 * ty + 32, z) for tx, ty in SLOTS), []), GREY))
    return HizScene(96, 96, stack[:n_stack // 2] + [Layer(occ, RED)] + stack[n_stack // 2:])


# hiz_depth_extremes: tile-covering occluders (SLOTS) at depth 1.0 (slot 0), 0.0 (slot 1) and clip z = -0.0 (slots 2,
# 3: its fragments store +0.0, DESIGN C5), with full-tile layers at the same depth drawn before (slots 0, 3) and after
# (slots 0, 1, 2): ties go to the later layer.  Small triangles pad slot 0 from behind and the others from in front.
def hiz_depth_extremes_geometry(seed=47):
    rng = np.random.default_rng(seed)
    zs = [1.0, 0.0, -0.0, -0.0]
    occ = [tile_occluder(tx, ty, z) for (tx, ty), z in zip(SLOTS, zs)]

    def tie_layer(k, z):
        tx, ty = SLOTS[k]
        return px_quad(32 * tx, 32 * ty, 32 * tx + 32, 32 * ty + 32, z)

    before = Layer(tie_layer(0, 1.0) + tie_layer(3, 0.0), BLUE)
    after = Layer(tie_layer(0, 1.0) + tie_layer(1, 0.0) + tie_layer(2, 0.0) + tie_layer(0, 0.5), GREEN)
    pad_back = _padding(rng, SLOTS[:1], 150, 0.05, 0.9)
    pad_front = _padding(rng, SLOTS[1:], 200, 0.05, 0.9, size=(0.6, 1.5))
    return HizScene(96, 96, [Layer(pad_back, GREY), before, Layer(occ, RED), after, Layer(pad_front, GREY)])


HIZ_GEOMETRY = {
    "hiz_occluder_edges": hiz_occluder_edges_geometry,
    "hiz_depth_margins": hiz_depth_margins_geometry,
    "hiz_deep_opaque_65": lambda: hiz_deep_opaque_geometry(33),
    "hiz_deep_opaque_129": lambda: hiz_deep_opaque_geometry(65),
    "hiz_deep_opaque_1025": lambda: hiz_deep_opaque_geometry(513),
    "hiz_deep_opaque_2100": lambda: hiz_deep_opaque_geometry(1050),
    "hiz_clipped_occluders": hiz_clipped_occluders_geometry,
    "hiz_depth_extremes": hiz_depth_extremes_geometry,
    # the stacks at a size that is not a multiple of 32 (the tiles at the right and bottom are cut), and under a
    # scissor that cuts tiles mid-row and mid-column
    "hiz_deep_opaque_odd_size": lambda: hiz_deep_opaque_geometry(720, w=53, h=45, seed=3),
    "hiz_deep_opaque_scissor": lambda: hiz_deep_opaque_geometry(720, seed=5, scissor=(5, 11, 50, 40)),
    "hiz_deep_opaque_rgba8": lambda: _rgba8(hiz_deep_opaque_geometry(160, seed=7)),
    "hiz_occluder_edges_rgba8": lambda: _rgba8(hiz_occluder_edges_geometry(seed=53)),
}


def _rgba8(sc):
    sc.color_format = A.COLOR_RGBA8
    return sc


SCENARIOS = {
    "shading_up": lambda lib: shading_constants(lib, (0, 1, 0)),
    "shading_side": lambda lib: shading_constants(lib, (1, 0, 0)),
    "shared_edge": shared_edge_additive,
    "fan": fan_additive,
    "depth_later_nearer": lambda lib: depth_order(lib, True),
    "depth_later_farther": lambda lib: depth_order(lib, False),
    "depth_tie": depth_tie,
    "transparent_layers": transparent_layers,
    "tex_nearest": lambda lib: textured_plane(lib, "nearest"),
    "tex_linear": lambda lib: textured_plane(lib, "linear"),
    "tex_trilinear": lambda lib: textured_plane(lib, "trilinear"),
    "tex_magnified": lambda lib: textured_plane(lib, "linear", tiles=0.11),
    "floor_trilinear": perspective_floor,
    "floor_nearest": lambda lib: perspective_floor(lib, sampler_kind="nearest"),
    "near_clip_wall": near_clip_wall,
    "depth_plane_85": lambda lib: depth_plane(lib, 85.0),
    "soup": random_soup,
    "soup_rgba8": lambda lib: random_soup(lib, color_format=A.COLOR_RGBA8, seed=11),
    "soup_opaque_only": lambda lib: random_soup(lib, seed=3, transparent_every=0, n_tris=900),
    "soup_scissor": lambda lib: random_soup(lib, seed=5, scissor=(13, 21, 101, 37)),
    "soup_odd_size": lambda lib: random_soup(lib, w=67, h=35, seed=9, n_tris=300),
    "transparent_stack_40": lambda lib: transparent_stack(lib, 40, jitter=0.05),
    # 2 * layers transparent triangles in one tile: from 100 layers up the tile is split into row quarters, and the
    # counting-rank sort runs with 1, 2, 4, 6 or 8 keys per thread
    "transparent_stack_100": lambda lib: transparent_stack(lib, 100, jitter=0.04),
    "transparent_stack_230": lambda lib: transparent_stack(lib, 230, jitter=0.03, seed=5),
    "transparent_stack_450": lambda lib: transparent_stack(lib, 450, jitter=0.02, seed=6),
    "transparent_stack_700": lambda lib: transparent_stack(lib, 700, jitter=0.02),
    "transparent_stack_1000": lambda lib: transparent_stack(lib, 1000, jitter=0.01, seed=8),
    # ~1000 opaque triangles per tile: split by the opaque term of the cost alone
    "soup_dense_split": lambda lib: random_soup(lib, w=96, h=64, seed=13, n_tris=6000, transparent_every=7),
    # ~9000 opaque triangles per tile: more than a quarter's row-filtered list holds in LDS (it walks the bin itself)
    "soup_very_dense_split": lambda lib: random_soup(lib, w=64, h=64, seed=17, n_tris=36000, transparent_every=9),
    "transparent_stack_1300_fallback": lambda lib: transparent_stack(lib, 1300),
    "transparent_stack_clipped": transparent_stack_clipped,
    "ragged": ragged_draws,
    "empty": empty_frame,
}
SCENARIOS.update({name: (lambda lib, make=make: render_hiz(lib, make())) for name, make in HIZ_GEOMETRY.items()})
