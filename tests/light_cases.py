"""Seeded cases for tests/light_geom_ref.py (family L) and the rig that draws them through a library of the svr.h ABI.

Every case is a handful of flat-shaded meshes (white 1 x 1 texture, a vertex colour and a colour factor per mesh), a
camera, a sun, an ambient colour and point lights; some add a shadow map drawn by a depth-only pass, a scissor, a row
interleave or the ambient-occlusion factor.  Everything about a case - its lights among it - is decided here, on the CPU,
from the reference's own surface points; no library runs.

  L1  the identity scene of family A (viewproj = I, w = 1): the inverse is exact, so the position carries the depth chain's
      error alone; the tight test of C19.
  L2  the projective scene of family D (position (x, y, w) -> clip (x, y, 9/8 - w/8, w), kept range 1 <= w <= 9).  The pass
      divides by h.w, so any multiple of the inverse serves; the one handed over, h = (9 xn, 9 yn, 9, 8 z + 1), is exact in
      float32 and not symmetric.  Triangles span w 1:8, one is cut by the near plane and one by the far plane.
  L3  real cameras (scenes.scene_data_struct) over the floor and the box of tests/test_lighting_gpu.py; the box's world
      matrix rotates and scales unevenly, so the stored normal is neither unit nor axis-aligned, and the floor crosses the
      near plane.  Both colour formats, an odd scissor, a row interleave, the ambient factor, three shadow cameras.
  L4  4096 lights over two tiles of the identity scene: about 64 reach a pixel, at indices that use the first and last bit
      of the first and last mask word and the second step of the 256-wide stride loop."""
import numpy as np

import __graft_entry__ as g
import light_geom_ref as LG
import lighting_ref as LR
import raster_cases as RC
import scenarios as SC
from test_lighting_gpu import FLOOR_X, FLOOR_Z, SHADOW_CAMERAS, SHADOW_SIZE  # the floor's extent and the light cameras: shared

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
f32 = np.float32

MIN_WINNERS = 512
LIGHT_CLEARANCE = 0.25  # world units between a light and every surface point it reaches
CLEAR = (0.0, 0.0, 0.0, 0.0)
PATTERN = (0.25, 0.5, 0.75, 0.125)  # a colour no lit pixel holds (alpha is not 1): what the pass must leave alone
# The shadow bias of each camera.  A nearest-texel map over a sloped receiver puts a lit pixel at a depth difference of up to
# half a texel's depth slope from its texel; unless the bias clears that, the lit floor flickers between the two answers
# from texel to texel, and every pixel whose window position is within its allowance of a texel boundary is offered either
# way.  The rule: the smallest power of two, from SHADOW_BIAS_FLOOR up (the order of the 2e-5 that the bit-exact shadow tests
# use), at which the reference, over the oracle's map, offers no more than a third of the cap (EITHER_OR_CAP / 3 of the
# winner pixels) either way.  tests/test_light_geom_ref.py holds each value to that rule and prints the counts.
SHADOW_BIAS_FLOOR = 2.0 ** -16
SHADOW_BIAS = {"covers_the_frame": 2.0 ** -16, "partly_outside": 2.0 ** -13, "behind_the_light": 2.0 ** -16}
CAMERAS = {"front": ((0.0, 2.5, 3.0), -0.12, 0.0), "oblique": ((-5.0, 4.0, 1.0), -0.3, -0.55), "down": ((3.0, 6.0, 0.0), -0.7, 0.4)}
LIGHTING = ((0.05, 0.2, 0.15, 1.0), (0.6, 0.3, -0.7, 0.0), (1.0, 0.9, 0.8, 0.7))  # ambient, sun direction, sun colour
L4_REACHING = (0, 31, 32, 255, 256, 4064, 4095)


# ---------------------------------------------------------------- the vertex stage in float32 (C0, C1)
def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum rounds twice (to 53 bits, then to 24), which
    differs from one rounding only when the first lands exactly on a float32 tie"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _chain(m, v):
    """m[col] (4,) float32, v (..., 4) float32 -> m v by the C0 chain"""
    r = m[0][None, :] * v[..., 0:1]
    for k in (1, 2, 3):
        r = _fma(np.broadcast_to(m[k][None, :], r.shape), np.broadcast_to(v[..., k:k + 1], r.shape), r)
    return r


def vertex_stage(viewproj, world, positions):
    """clip coordinates (n, 4) float32 as C0/C1 compute them: mvp = viewproj x world column by column, then mvp (p, 1)"""
    vp, wm = np.asarray(viewproj, f32).reshape(4, 4), np.asarray(world, f32).reshape(4, 4)
    mvp = _chain(vp, wm)
    p1 = np.concatenate([np.asarray(positions, f32), np.ones((len(positions), 1), f32)], axis=1)
    return _chain(mvp, p1)


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, name, family, width, height, scene, meshes, lighting=LIGHTING, fmt=A.COLOR_RGBA16F, inv_viewproj=None,
                 scissor=None, interleave=(1, 0), shadow=None, ao=False, bounds=None, n_lights=24, seed=0, reach=(1.5, 6.0)):
        """meshes: [(positions (n, 3), normals (n, 3), vertex colour (4,), colour factor (4,), world 4 x 4 [col][row])]"""
        self.name, self.family, self.width, self.height, self.scene, self.fmt = name, family, width, height, scene, fmt
        self.raw = [(np.asarray(p, f32), np.asarray(n, f32), np.asarray(c, f32), np.asarray(k, f32), np.asarray(w, f32)) for p, n, c, k, w in meshes]
        self.ambient, self.sun_dir, self.sun_color = (np.array(v, f32) for v in lighting)
        self.viewproj = LR.m16(scene.viewproj)
        self.inv_viewproj = LR.inv_viewproj(scene.viewproj) if inv_viewproj is None else LR.m16(inv_viewproj)
        self.scissor, self.interleave, self.shadow, self.ao, self.bounds = scissor, interleave, shadow, ao, bounds
        self.meshes = [LG.Mesh(p, n, c.astype(np.float64) * k.astype(np.float64), w.reshape(16), vertex_stage(self.viewproj, w, p))
                       for p, n, c, k, w in self.raw]
        self.owned = LR.owned_mask(width, height, scissor, interleave)
        self.lights = np.zeros(0, A.POINT_LIGHT_DTYPE)
        if n_lights:
            self.lights = self._lights(n_lights, seed, reach)

    def lighting(self, shadow=None, ao=None, lights=None, bias=None):
        """the reference's inputs; shadow and ao are the planes as a library holds them"""
        sh = dict(shadow=shadow, shadow_viewproj=LR.m16(shadow_scene(self.shadow).viewproj),
                  bias=SHADOW_BIAS[self.shadow] if bias is None else bias) if shadow is not None else {}
        return LG.Lighting(self.inv_viewproj, self.ambient, self.sun_dir, self.sun_color, self.lights if lights is None else lights, ao=ao, **sh)

    def reference(self, shadow=None, ao=None, lights=None, bias=None):
        return LG.render(self.width, self.height, self.viewproj, self.meshes, self.lighting(shadow, ao, lights, bias), self.fmt)

    def _lights(self, n, seed, reach):
        """n seeded lights above surface points of the reference (along the stored normal, so that n . v > 0 around them), kept
        LIGHT_CLEARANCE off every surface point they reach; radii log-uniform over `reach`"""
        ref = self.reference(lights=np.zeros(0, A.POINT_LIGHT_DTYPE))
        own = self.owned[ref.ys, ref.xs]
        rng = np.random.default_rng(seed)
        L = np.zeros(n, A.POINT_LIGHT_DTYPE)
        k = 0
        while k < n:
            i = int(rng.choice(np.nonzero(own)[0]))
            nrm = ref.normal[i] / np.linalg.norm(ref.normal[i])
            radius = f32(np.exp(rng.uniform(np.log(reach[0]), np.log(reach[1]))))
            pos = (ref.P[i] + nrm * rng.uniform(0.3, 0.6) * float(radius) + rng.normal(0, 0.05, 3) * float(radius)).astype(f32)
            d = np.linalg.norm(ref.P - pos.astype(np.float64)[None, :], axis=1)
            if d.min() < LIGHT_CLEARANCE or not (d[own] < 0.9 * float(radius)).any():
                continue
            L["position"][k], L["radius"][k] = pos, radius
            L["color"][k], L["intensity"][k] = rng.uniform(0.2, 1.0, 3).astype(f32), f32(rng.uniform(0.5, 4.0))
            k += 1
        return L


def shadow_scene(which):
    pos, pitch, yaw = SHADOW_CAMERAS[which]
    return S.scene_data_struct(pos, pitch, yaw, *SHADOW_SIZE)


def _normals(rng, n, towards):
    """per-vertex normals of random length 0.5 .. 2 within ~50 degrees of `towards`"""
    v = np.asarray(towards, np.float64)[None, :] + rng.uniform(-0.6, 0.6, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(f32)


def _flat_triangles(rng, width, height, count, scene_kind, values):
    """`count` large seeded triangles: window positions over the target (and a little beyond), z (identity scene) or w
    (near/far scene) per vertex from `values`; positions (3 count, 3) float32 in the scene's own space"""
    pos = []
    for k in range(count):
        while True:
            xy = rng.uniform((-0.1 * width, -0.1 * height), (1.1 * width, 1.1 * height), (3, 2))
            area = abs((xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[2, 0] - xy[0, 0]) * (xy[1, 1] - xy[0, 1]))
            if area >= 0.5 * width * height:
                break
        clip = RC._clip_d(xy, values(k), width, height, scene_kind)
        pos.append(clip[:, [0, 1, 3]] if scene_kind == "nearfar" else clip[:, :3])
    return np.concatenate(pos)


def family_l1(seed=8101):
    cases = []
    for (w, h), n in (((64, 48), 40), ((33, 35), 8)):
        rng = np.random.default_rng(seed + w)
        pos = _flat_triangles(rng, w, h, 4, "identity", lambda k: np.round(rng.uniform(0.1, 0.9, 3) * 256) / 256)
        meshes = [(pos[3 * k:3 * k + 3], _normals(rng, 3, (0, 0, 1)), rng.uniform(0.3, 1.0, 4), rng.uniform(0.5, 1.0, 4), SC.IDENT) for k in range(4)]
        cases.append(Case(f"L1-{w}x{h}", "L1", w, h, SC.identity_scene(), meshes, inv_viewproj=SC.IDENT, n_lights=n, seed=seed, reach=(0.4, 1.5),
                          bounds=dict(extents=RC.BIG)))
    return cases


def nearfar_scene():
    nf = np.zeros((4, 4), dtype=f32)
    nf[0][0] = nf[1][1] = 1
    nf[2][2], nf[3][2], nf[2][3] = -0.125, 1.125, 1
    return A.scene_struct(SC.IDENT, SC.IDENT, nf, [0.0] * 4, (0, 1, 0, 1), (1, 1, 1, 1))


def family_l2(seed=8202):
    inv = np.zeros((4, 4), f32)  # [col][row]: h = (9 xn, 9 yn, 9, 8 z + 1)
    inv[0][0] = inv[1][1] = 9
    inv[3][2], inv[2][3], inv[3][3] = 9, 8, 1
    cases = []
    for (w, h), n in (((64, 48), 24), ((33, 35), 12)):
        rng = np.random.default_rng(seed + w)
        spans = [(1.25, 4.0, 8.5), (8.0, 1.5, 3.0), (0.5, 3.0, 6.0), (11.0, 5.0, 2.0)]  # w 1:8; one beyond the near plane, one beyond the far plane
        pos = _flat_triangles(rng, w, h, 4, "nearfar", lambda k: spans[k])
        meshes = [(pos[3 * k:3 * k + 3], _normals(rng, 3, (0, 0, -1)), rng.uniform(0.3, 1.0, 4), rng.uniform(0.5, 1.0, 4), SC.IDENT) for k in range(4)]
        cases.append(Case(f"L2-{w}x{h}", "L2", w, h, nearfar_scene(), meshes, inv_viewproj=inv, n_lights=n, seed=seed, reach=(1.0, 5.0),
                          bounds=dict(origin=(0, 0, 5), extents=(1e6, 1e6, 4.5))))
    return cases


BOX_WORLD = GL.scale(GL.rotate(GL.translate(GL.identity(), (0.5, 1.75, -7.0)), 0.5, (0.3, 1.0, 0.2)), (2.5, 1.5, 2.0))


def flat_floor_and_box():
    """the floor (y = 0) and the box above it of tests/test_lighting_gpu.py as flat meshes; the box turned and scaled unevenly"""
    (x0, x1), (z0, z1) = FLOOR_X, FLOOR_Z
    quad = np.array([(x0, 0, z1), (x1, 0, z1), (x1, 0, z0), (x0, 0, z0)], f32)[SC.QUAD_IDX]
    cube = S.cube_mesh()
    v = cube.vertices[cube.indices]
    return [(quad, np.tile(np.array([0, 1, 0], f32), (6, 1)), (0.8, 0.7, 0.6, 1.0), (1.0, 1.0, 1.0, 1.0), GL.identity()),
            (v["position"], v["normal"], (0.9, 0.5, 0.7, 1.0), (0.7, 0.9, 0.6, 1.0), BOX_WORLD)]


def family_l3():
    def case(name, cam, size=(64, 48), **kw):
        pos, pitch, yaw = CAMERAS[cam]
        return Case(f"L3-{name}", "L3", size[0], size[1], S.scene_data_struct(pos, pitch, yaw, *size), flat_floor_and_box(), **kw)

    return [case("front", "front", seed=31),
            case("oblique-rgba8-33x35", "oblique", size=(33, 35), fmt=A.COLOR_RGBA8, seed=32),
            case("oblique", "oblique", seed=33),
            case("front-rgba8", "front", fmt=A.COLOR_RGBA8, seed=34),
            case("scissor", "down", scissor=(5, 3, 41, 29), seed=35),
            case("interleave", "front", interleave=(3, 1), seed=36),
            case("ao", "front", ao=True, seed=37)]


def family_l3_shadow():
    return [Case(f"L3-shadow-{which}", "L3s", 64, 48, S.scene_data_struct(*CAMERAS["down"], 64, 48), flat_floor_and_box(), shadow=which, seed=41 + k)
            for k, which in enumerate(sorted(SHADOW_CAMERAS))]


def family_l4(seed=8404):
    """64 x 32, the identity scene, SVR_MAX_LIGHTS lights: the reaching ones at L4_REACHING and at seeded indices between"""
    w, h = 64, 32
    rng = np.random.default_rng(seed)
    pos = _flat_triangles(rng, w, h, 3, "identity", lambda k: np.round(rng.uniform(0.1, 0.9, 3) * 256) / 256)
    meshes = [(pos[3 * k:3 * k + 3], _normals(rng, 3, (0, 0, 1)), rng.uniform(0.3, 1.0, 4), rng.uniform(0.5, 1.0, 4), SC.IDENT) for k in range(3)]
    c = Case("L4-4096", "L4", w, h, SC.identity_scene(), meshes, inv_viewproj=SC.IDENT, n_lights=64, seed=seed, reach=(0.4, 1.0), bounds=dict(extents=RC.BIG))
    reaching = c.lights
    n = A.MAX_LIGHTS
    idx = np.array(sorted(set(L4_REACHING) | set(rng.choice(np.arange(33, 4064), 64 - len(L4_REACHING), replace=False).tolist())))
    assert len(idx) == 64
    L = np.zeros(n, A.POINT_LIGHT_DTYPE)
    # the rest: beside the scene, with radii that reach nothing
    L["position"] = rng.uniform((-1, -1, 3.0), (1, 1, 4.0), (n, 3)).astype(f32)
    L["radius"], L["color"], L["intensity"] = rng.uniform(0.01, 0.5, n).astype(f32), rng.uniform(0.2, 1.0, (n, 3)).astype(f32), 1.0
    L[idx] = reaching
    c.lights, c.reaching = L, idx
    return [c]


_CACHE = {}


def cases(family):
    if family not in _CACHE:
        _CACHE[family] = {"L1": family_l1, "L2": family_l2, "L3": family_l3, "L3s": family_l3_shadow, "L4": family_l4}[family]()
    return _CACHE[family]


FAMILIES = ("L1", "L2", "L3", "L3s", "L4")


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]


# ---------------------------------------------------------------- the rig
def _bounds(positions):
    lo, hi = positions.min(axis=0), positions.max(axis=0)
    return dict(origin=tuple((lo + hi) / 2), extents=tuple((hi - lo) / 2))


class Rig:
    """one context: the case's meshes under a white 1 x 1 texture"""

    def __init__(self, lib, case, width=None, height=None, fmt=None):
        self.case = case
        self.r = lib.create(width or case.width, height or case.height, case.fmt if fmt is None else fmt)
        white = self.r.create_image(S.white_1x1())
        smp = self.r.create_sampler(**S.SAMPLER_LINEAR)
        ros = []
        for p, n, c, k, w in case.raw:
            verts = SC.make_vertices(p, n, colors=np.tile(c, (len(p), 1)))
            mesh = self.r.upload_mesh(np.arange(len(p), dtype=np.uint32), verts)
            mat = self.r.write_material(A.PASS_MAIN_COLOR, tuple(float(x) for x in k), white, smp)
            ros.append(SC.render_object(mesh, mat, 0, len(p), transform=w, **(case.bounds or _bounds(p))))
        self.objects = SC.objs(ros)

    def draw(self, scene=None):
        """the geometry pass over a target cleared to zero alpha -> covered (alpha written), depth"""
        self.r.clear_color(CLEAR)
        self.r.draw_geometry(scene or self.case.scene, self.objects)
        color = self.r.read_color()
        alpha = color[..., 3] != 0
        return alpha, self.r.read_depth()

    def close(self):
        self.r.close()


def shadow_map(lib, case, depth_only):
    """the case's shadow map as `lib` draws it, by a depth-only pass or (the oracle has none) as the depth of a geometry pass
    -> (Rig that holds it, the plane as read back)"""
    rig = Rig(lib, case, *SHADOW_SIZE, fmt=A.COLOR_RGBA16F)
    if depth_only:
        rig.r.draw_depth(shadow_scene(case.shadow), rig.objects)
        rig.r.sync()
    else:
        rig.r.draw_geometry(shadow_scene(case.shadow), rig.objects)
    return rig, rig.r.read_depth()
