"""Seeded cases for tests/raster_ref.py and the rig that draws them through a library of the svr.h ABI.

Every case is one svr_draw_geometry pass: full scissor, identity world matrix, white vertex colour, colour factors 1,
normal and sun (0, 1, 0), ambient 0, sun intensity 1 - so the light term is 1, colour is the texel and the ALBEDO plane is
the fp32 texel.  Family A uses viewproj = identity (clip = position, w = 1).  Families B and C use a viewproj whose
last row takes w from the position's z: position (x, y, w) -> clip (x, y, w/4 + 1/8, w); every product and sum of that
C0/C1 chain is exact for the values used (x, y pass through; w is a multiple of 2^-8 in [1/4, 16]), so the clip
coordinates the reference is handed are the ones the libraries compute.

Family D is the clip volume and the guard band (C2): triangles that cross z = w (the near plane under reversed Z) and
z = 0 with one vertex and with two, both planes at once, vertices with w < 0 and w = 0, triangles wholly outside, vertices
and edges exactly on a plane, vertices up to 10^6 px beyond the guard band with controls just inside it, and pairs that
share an edge a plane cuts.  It uses the identity scene (w = 1, z straight from the position) and a second projective
scene, position (x, y, w) -> clip (x, y, 9/8 - w/8, w), whose kept range is 1 <= w <= 9; that chain is exact too."""
import numpy as np

import __graft_entry__ as g
import image_ref as IR
import raster_ref as RR
import scenarios as SC

pkg = g.load_package()
A = pkg.abi
f32 = np.float32
BIG = (1e6, 1e6, 1e6)  # bounds that is_visible never culls
TRACED = 32            # covered pixels traced per case (all of them where a case covers fewer); the least a case of B-D covers
EITHER_OR_CAP = 0.01   # of a case's covered pixels: the share an either/or rule may be offered at


class Case:
    def __init__(self, name, family, width, height, tris, tex="white", mipmapped=False, smp=(0, 0, 0, 0.0, 0.0),
                 projective=True, exact=False, pair=False):
        self.name, self.family, self.width, self.height = name, family, width, height
        self.tris = tris  # [(clip (3, 4) f32, uv (3, 2) f32)]
        self.tex, self.mipmapped, self.smp, self.projective, self.exact, self.pair = tex, mipmapped, smp, projective, exact, pair
        # projective: False = the identity scene, True = z = w/4 + 1/8, "nearfar" = z = 9/8 - w/8 (family D)


def _clip_from_window(xy_px, w, width, height, projective):
    """window positions in pixels (float64) and w -> clip float32 (n, 4)"""
    xy_px, w = np.asarray(xy_px, np.float64), np.asarray(w, np.float64)
    ndc = np.stack([xy_px[:, 0] * 2.0 / width - 1.0, xy_px[:, 1] * 2.0 / height - 1.0], axis=1)
    clip = np.zeros((len(w), 4), f32)
    clip[:, 0], clip[:, 1] = (ndc[:, 0] * w).astype(f32), (ndc[:, 1] * w).astype(f32)
    clip[:, 3] = w.astype(f32)
    clip[:, 2] = (f32(0.25) * clip[:, 3] + f32(0.125)) if projective else f32(0.5)
    if projective:  # the chain fma(1/8, 1, 1/4 * w) is exact
        assert np.all(clip[:, 2].astype(np.float64) == 0.25 * clip[:, 3].astype(np.float64) + 0.125)
    return clip


# ---------------------------------------------------------------- family A: coverage
def _grid_coord(rng, lo_px, hi_px):
    """a coordinate in 1/256 pixel, weighted towards pixel corners (multiples of 256) and centres (128 mod 256)"""
    kind = rng.integers(0, 10)
    p = int(rng.integers(lo_px, hi_px))
    if kind < 4:
        return p * 256
    if kind < 7:
        return p * 256 + 128
    return p * 256 + int(rng.integers(0, 256))


def family_a(width, height, seed):
    """~150 single triangles per target (w = 1, vertices on the 1/256 grid), each with both windings; pairs that share
    an edge follow each other (pair=True on the second)."""
    rng = np.random.default_rng(seed)
    shapes = []  # (kind, three (X, Y) in 1/256 px)
    P = lambda m=0: (_grid_coord(rng, -m, width + m), _grid_coord(rng, -m, height + m))
    for _ in range(24):
        shapes.append(("random", [P(), P(), P()]))
    for _ in range(10):  # up to 200 px outside the target: inside the guard band, no clipping
        shapes.append(("outside", [P(200), P(200), P(4)]))
    for _ in range(10):  # slivers thinner than a pixel
        a, b = P(), P()
        k = rng.integers(1, 200)
        shapes.append(("sliver", [a, b, ((a[0] + b[0]) // 2 + int(rng.integers(-k, k + 1)), (a[1] + b[1]) // 2 + int(rng.integers(-k, k + 1)))]))
    for _ in range(6):  # zero area: collinear or repeated vertices
        a, b = P(), P()
        shapes.append(("zero", [a, b, (2 * b[0] - a[0], 2 * b[1] - a[1])] if rng.integers(0, 2) else [a, b, a]))
    for _ in range(8):  # a horizontal and a vertical edge, through centres or along boundaries
        a, c = P(), P()
        shapes.append(("axis", [a, (c[0], a[1]), (a[0], c[1])]))
    for _ in range(6):  # edges exactly through pixel centres: vertices on centres, 45 degrees
        x, y, s = int(rng.integers(2, width - 12)), int(rng.integers(2, height - 12)), int(rng.integers(3, 10))
        a = (x * 256 + 128, y * 256 + 128)
        shapes.append(("diag", [a, (a[0] + s * 256, a[1] + s * 256), (a[0] + s * 256, a[1] - 256 * int(rng.integers(0, 3)))]))
    cases = []
    for k, (kind, v) in enumerate(shapes):
        for wind in (0, 1):
            vv = v if wind == 0 else [v[0], v[2], v[1]]
            cases.append(_case_a(f"A{width}x{height}-{kind}{k}-{wind}", vv, width, height))
    for k in range(10):  # pairs sharing an edge: the quad a, b, c, d cut along a-c
        a, b, c, d = P(2), P(2), P(2), P(2)
        side = lambda p: (c[0] - a[0]) * (p[1] - a[1]) - (p[0] - a[0]) * (c[1] - a[1])
        while side(b) == 0 or side(b) * side(d) >= 0:  # b and d on opposite sides of a-c: the halves do not overlap
            b, d = P(2), P(2)
        cases.append(_case_a(f"A{width}x{height}-pair{k}-0", [a, b, c], width, height))
        second = _case_a(f"A{width}x{height}-pair{k}-1", [c, d, a] if k % 2 else [a, c, d], width, height)
        second.pair = True
        cases.append(second)
    return cases


def _case_a(name, v, width, height):
    xy = np.array(v, np.float64) / 256.0
    clip = _clip_from_window(xy, np.ones(3), width, height, projective=False)
    X, Y, _, _, _ = RR.snap(clip, width, height)
    assert [tuple(p) for p in zip(X.tolist(), Y.tolist())] == [tuple(p) for p in v], "family A vertices snap to themselves"
    c = Case(name, "A", width, height, [(clip, np.full((3, 2), 0.5, f32))], projective=False)  # uv: the centre of the white texel
    c.grid = v
    return c


# ---------------------------------------------------------------- family B: interpolation
def _off_tie(clip, width, height):
    return RR.snap(clip, width, height)[4].min() >= 2.0 ** -4


def family_b(seed=7202, count=60, width=64, height=48):
    """Single triangles, w per vertex over ratios up to 1:64, vertices off the grid and strictly inside the clip volume;
    a vertex whose window coordinate * 256 lies within 2^-4 of a rounding tie is drawn again."""
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < count:
        xy = rng.uniform((1.0, 1.0), (width - 1.0, height - 1.0), (3, 2))
        top = 2.0 ** rng.uniform(0, 6)  # ratio of the largest to the smallest w, up to 64
        w = np.round(0.25 * top ** rng.uniform(0, 1, 3) * 256) / 256
        w[rng.integers(0, 3)] = 0.25
        w[(rng.integers(0, 3))] = np.round(0.25 * top * 256) / 256
        clip = _clip_from_window(xy, w, width, height, True)
        area = abs((xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[2, 0] - xy[0, 0]) * (xy[1, 1] - xy[0, 1]))
        if not _off_tie(clip, width, height) or area < 80.0 or np.any(np.abs(clip[:, :2]) >= clip[:, 3:4] * 0.999):
            continue
        uv = rng.uniform(-8, 8, (3, 2)).astype(f32)
        cases.append(Case(f"B{len(cases)}", "B", width, height, [(clip, uv)], tex="r16x16", mipmapped=False,
                          smp=(RR.LINEAR, RR.LINEAR, RR.NEAREST, 0.0, 0.0)))
    return cases


# ---------------------------------------------------------------- family C: the texture unit
TEXTURES = {"r16x16": (16, 16), "r8x4": (8, 4), "r5x3": (5, 3), "r1x7": (1, 7), "r1x1": (1, 1), "white": (1, 1)}
LOD_CLAMPS = ((0.0, 0.0), (1.5, 2.25), (0.0, 1000.0))


def texture(name):
    w, h = TEXTURES[name]
    if name == "white":
        return np.full((1, 1, 4), 255, np.uint8)
    rng = np.random.default_rng(1000 + 16 * w + h)
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def _quad(rng, ratio, aniso, projective, width=64, height=48):
    """A quad (two triangles sharing a diagonal) whose uv advance `ratio` texels of a 16-texel level per pixel along x
    and the same (isotropic) or an eighth of it along y, rotated in uv by a random angle; w = 1, or 1 on the left and 2-4
    on the right edge.  uv stays inside [-8, 8] and crosses 0."""
    while True:
        rate_x, rate_y = ratio / 16.0, ratio / 16.0 / (8.0 if aniso else 1.0)
        wpx, hpx = float(np.clip(10.0 / rate_x, 6.0, 52.0)), float(np.clip(10.0 / rate_y, 6.0, 38.0))
        x0, y0 = rng.uniform(2.0, width - 2.0 - wpx), rng.uniform(2.0, height - 2.0 - hpx)
        shear = rng.uniform(-0.08, 0.08) * hpx
        xy = np.array([(x0, y0), (x0 + wpx, y0 + shear), (x0 + wpx, y0 + hpx + shear), (x0, y0 + hpx)])
        xy = np.clip(xy, 1.0, (width - 1.0, height - 1.0))
        wr = float(rng.integers(2, 5)) if projective else 1.0
        w = np.array([1.0, wr, wr, 1.0])
        ang = rng.uniform(0, 2 * np.pi) if rng.integers(0, 2) else 0.0
        su, sv = rate_x * wpx, rate_y * hpx
        base = np.array([(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]) * (su, sv)
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        uv = (base @ rot.T + rng.uniform(-0.7, 0.7, 2)).astype(f32)
        clip = _clip_from_window(xy, w, width, height, True)
        if _off_tie(clip, width, height) and np.abs(uv).max() < 8.0:
            idx = ([0, 1, 2], [0, 2, 3])
            return [(clip[i], uv[i]) for i in idx]


def family_c(seed=9107):
    """Every texture (mip-mapped and not) x the eight samplers x three LOD clamps, each on one of sixteen seeded quads:
    ratios 0.1 - 20 texels per pixel, isotropic and 8:1, affine and projective.  Then the exact cases."""
    rng = np.random.default_rng(seed)
    ratios = 0.1 * 200.0 ** (np.arange(16) / 15.0)
    geoms = [_quad(rng, float(ratios[k]), aniso=bool(k & 1), projective=bool((k >> 1) & 1)) for k in range(16)]
    cases, n = [], 0
    for tex in ("r16x16", "r8x4", "r5x3", "r1x7", "r1x1"):
        for mipmapped in (True, False):
            for mag in (0, 1):
                for minf in (0, 1):
                    for mip in (0, 1):
                        for lo, hi in LOD_CLAMPS:
                            k = (5 * n + n // 16) % 16
                            cases.append(Case(f"C-{tex}{'m' if mipmapped else ''}-{mag}{minf}{mip}-{lo}-{hi}-g{k}", "C", 64, 48,
                                              geoms[k], tex=tex, mipmapped=mipmapped, smp=(mag, minf, mip, lo, hi)))
                            n += 1
    # exact: w = 1, a 16 x 16 pixel quad on the grid, texels 1:1 on pixels (rho^2 = 1, lambda = 0: the MAG filter) and
    # 2:1 (lambda = 1), shifted by a quarter texel so that LINEAR and NEAREST differ at every pixel
    for scale, tag in ((1.0, "1to1"), (2.0, "2to1")):
        xy = np.array([(8.0, 16.0), (24.0, 16.0), (24.0, 32.0), (8.0, 32.0)])
        q = 0.25 / 16.0
        uv = (np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float64) * scale + q).astype(f32)
        clip = _clip_from_window(xy, np.ones(4), 64, 48, True)
        tris = [(clip[i], uv[i]) for i in ([0, 1, 2], [0, 2, 3])]
        for mag in (0, 1):
            for minf in (0, 1):
                for mip in (0, 1):
                    cases.append(Case(f"C-exact{tag}-{mag}{minf}{mip}", "C", 64, 48, tris, tex="r16x16", mipmapped=True,
                                      smp=(mag, minf, mip, 0.0, 1000.0), exact=True))
    return cases


# ---------------------------------------------------------------- family D: the clip volume and the guard band
TRILINEAR = (RR.LINEAR, RR.LINEAR, RR.LINEAR, 0.0, 1000.0)
D_GROUPS = ("near1", "near2", "far1", "far2", "both", "wneg", "empty", "onplane", "guard", "control", "pair")


def _clip_d(xy_px, zw, width, height, scene):
    """window positions in pixels and, per vertex, z (identity scene, w = 1) or w (the near/far scene, a multiple of
    2^-8; w < 0 mirrors the position through the centre, as the projection does) -> clip float32 (3, 4)"""
    xy_px, zw = np.asarray(xy_px, np.float64), np.asarray(zw, np.float64)
    ndc = np.stack([xy_px[:, 0] * 2.0 / width - 1.0, xy_px[:, 1] * 2.0 / height - 1.0], axis=1)
    clip = np.zeros((3, 4), f32)
    if scene == "nearfar":
        w = np.round(zw * 256.0) / 256.0
        clip[:, 0], clip[:, 1] = (ndc[:, 0] * np.where(w == 0, 1.0, w)).astype(f32), (ndc[:, 1] * np.where(w == 0, 1.0, w)).astype(f32)
        clip[:, 3] = w.astype(f32)
        clip[:, 2] = f32(-0.125) * clip[:, 3] + f32(1.125)
        # the chain fma(9/8, 1, -1/8 * w) is exact, and x, y, w pass through
        assert np.all(clip[:, 3].astype(np.float64) == w) and np.all(clip[:, 2].astype(np.float64) == 1.125 - 0.125 * w)
    else:
        clip[:, 0], clip[:, 1], clip[:, 2], clip[:, 3] = ndc[:, 0].astype(f32), ndc[:, 1].astype(f32), zw.astype(f32), f32(1.0)
    return clip


def _d_value(rng, scene, where):
    """z (identity) or w (near/far scene) of a vertex that is inside the volume, beyond z = w ("near"), beyond z = 0
    ("far"), behind the eye or on the eye plane (near/far scene only), or exactly on a plane"""
    if scene == "nearfar":
        lo, hi = {"in": (1.25, 8.5), "near": (0.125, 0.875), "far": (9.5, 12.0), "neg": (-2.0, -0.125), "zero": (0.0, 0.0),
                  "on_near": (1.0, 1.0), "on_far": (9.0, 9.0)}[where]
    else:
        lo, hi = {"in": (0.0625, 0.9375), "near": (1.0625, 2.0), "far": (-1.0, -0.0625), "on_near": (1.0, 1.0), "on_far": (0.0, 0.0)}[where]
    return float(np.round(rng.uniform(lo, hi) * 256.0) / 256.0)


def _d_accept(clip, uv, width, height, want_clipped=True, empty=False):
    """the reference alone decides whether a drawn candidate is kept: routed as meant, enough ideal coverage, and the
    offered share under the cap"""
    if RR.routed_to_clipper(clip, width, height) != want_clipped:
        return False
    if not want_clipped:
        t = RR.Tri(clip, uv, width, height)
        return _off_tie(clip, width, height) and int(t.coverage().sum()) >= TRACED
    t = RR.ClippedTri(clip, uv, width, height)
    n = int(t.coverage().sum())
    if empty:
        return n == 0 and not t.offered().any()
    return n >= TRACED and int(t.offered().sum()) <= EITHER_OR_CAP * n


def _d_uv(rng, textured):
    return rng.uniform(-4.0, 4.0, (3, 2)).astype(f32) if textured else np.full((3, 2), 0.5, f32)


def family_d(seed=6203):
    """~200 cases, a third textured through r16x16 with a trilinear sampler; both windings of every shape."""
    rng = np.random.default_rng(seed)
    cases = []

    def add(group, clip, uv, width, height, scene, textured, pair=False, both_windings=True):
        for wind in ((0, 1) if both_windings else (0,)):
            o = [0, 1, 2] if wind == 0 else [0, 2, 1]
            k = sum(c.name.startswith(f"D-{group}-") for c in cases)
            c = Case(f"D-{group}-{k}", "D", width, height, [(clip[o].copy(), uv[o].copy())], projective=("nearfar" if scene == "nearfar" else False),
                     **(dict(tex="r16x16", mipmapped=True, smp=TRILINEAR) if textured else {}))
            c.group, c.pair, c.clipped, c.empty = group, pair, RR.routed_to_clipper(clip, width, height), group == "empty"
            cases.append(c)

    def draw(group, wheres, scene, width=64, height=48, spread=1.0, empty=False, textured=False, clipped=True):
        while True:
            xy = rng.uniform((-spread * width, -spread * height), ((1 + spread) * width, (1 + spread) * height), (3, 2))
            zw = [_d_value(rng, scene, wh) for wh in wheres]
            clip = _clip_d(xy, zw, width, height, scene)
            if any(wh == "zero" for wh in wheres):  # no window position: a direction
                for i, wh in enumerate(wheres):
                    if wh == "zero":
                        clip[i, 0], clip[i, 1] = f32(rng.uniform(-3, 3)), f32(rng.uniform(-3, 3))
            uv = _d_uv(rng, textured)
            if _d_accept(clip, uv, width, height, clipped, empty):
                return clip, uv

    n = [0]

    def tex():  # every third shape
        n[0] += 1
        return n[0] % 3 == 0

    for group, wheres in (("near1", ("near", "in", "in")), ("near2", ("near", "near", "in")),
                          ("far1", ("far", "in", "in")), ("far2", ("far", "far", "in"))):
        for k in range(8):
            scene, t = ("identity", "nearfar")[k & 1], tex()
            order = list(rng.permutation(3))
            clip, uv = draw(group, [wheres[i] for i in order], scene, textured=t, spread=0.6)
            add(group, clip, uv, 64, 48, scene, t)
    for k in range(10):  # both planes: polygons of 5 to 7 vertices
        scene, t = ("identity", "nearfar")[k & 1], tex()
        wheres = [("near", "far", "in"), ("near", "far", "far"), ("near", "near", "far")][k % 3]
        order = list(rng.permutation(3))
        clip, uv = draw("both", [wheres[i] for i in order], scene, textured=t, spread=0.6)
        add("both", clip, uv, 64, 48, scene, t)
    for k in range(12):  # behind the eye and on the eye plane
        t = tex()
        wheres = [("neg", "in", "in"), ("neg", "neg", "in"), ("zero", "in", "in"), ("neg", "far", "in"), ("zero", "neg", "in"), ("neg", "in", "far")][k % 6]
        order = list(rng.permutation(3))
        clip, uv = draw("wneg", [wheres[i] for i in order], "nearfar", textured=t, spread=0.4)
        add("wneg", clip, uv, 64, 48, "nearfar", t)
    for k in range(6):  # wholly beyond a plane, or behind the eye: nothing is drawn and nothing offered
        scene = ("identity", "nearfar")[k & 1]
        wheres = [("near",) * 3, ("far",) * 3, ("neg",) * 3 if scene == "nearfar" else ("far",) * 3][k % 3]
        clip, uv = draw("empty", wheres, scene, empty=True, spread=0.2)
        add("empty", clip, uv, 64, 48, scene, False)
    for k in range(8):  # a vertex exactly on a plane beside one beyond it; an edge lying in a plane
        scene, t = ("identity", "nearfar")[k & 1], tex()
        wheres = [("on_near", "near", "in"), ("on_far", "far", "in"), ("on_near", "on_near", "in"), ("on_far", "on_far", "near"),
                  ("on_near", "far", "in"), ("on_far", "near", "in"), ("on_near", "on_near", "far"), ("on_far", "on_far", "in")][k]
        clipped = not (set(wheres) <= {"on_near", "on_far", "in"})
        clip, uv = draw("onplane", wheres, scene, textured=t, spread=0.5, clipped=clipped)
        add("onplane", clip, uv, 64, 48, scene, t)
    # guard band, on the 32 x 32 target: one or two vertices 16 385 to 10^6 px out in x, in y, in both, all of w > 0;
    # controls 16 000 to 16 383 px out keep the exact path.  Far coordinates are multiples of 1/256 px and their w a
    # power of two, so that x_s (and its snap) is the same number in float32 and float64: ndc = (256 x_s - 4096) / 4096.
    def guard(group, lo, hi, count):
        for k in range(count):
            scene, t = ("identity", "nearfar")[k & 1], tex()
            axes, two = ("x", "y", "xy")[k % 3], (k // 3) & 1
            while True:
                xy = rng.uniform((2.0, 2.0), (30.0, 30.0), (3, 2))
                xy = np.round(xy * 256.0) / 256.0
                zw = [_d_value(rng, scene, "in") for _ in range(3)]
                for i in range(1 + two):
                    far = np.round(np.exp(rng.uniform(np.log(lo), np.log(hi))) * 256.0) / 256.0
                    for a, ch in enumerate("xy"):
                        if ch in axes:
                            xy[i, a] = far * (1 if rng.integers(0, 2) else -1)
                    if scene == "nearfar":
                        zw[i] = float(2.0 ** rng.integers(1, 4))
                clip = _clip_d(xy, zw, 32, 32, scene)
                uv = _d_uv(rng, t)
                if _d_accept(clip, uv, 32, 32, want_clipped=(group == "guard")):
                    break
            add(group, clip, uv, 32, 32, scene, t)

    guard("guard", 16385.0, 1.0e6, 12)
    guard("control", 16000.0, 16383.0, 6)
    # pairs sharing an edge that a plane cuts: the quad a, b, c, d cut along a-c, a inside and c beyond a plane; a pass
    # each, the shared edge running a -> c in one and c -> a (odd k) or a -> c (even k) in the other
    for k in range(12):
        scene, t = ("identity", "nearfar")[k & 1], tex()
        beyond = ("near", "far", "neg" if scene == "nearfar" else "near")[k % 3]
        while True:
            xy = rng.uniform((-0.3 * 64, -0.3 * 48), (1.3 * 64, 1.3 * 48), (4, 2))
            a, b, c, d = xy
            side = lambda p: (c[0] - a[0]) * (p[1] - a[1]) - (p[0] - a[0]) * (c[1] - a[1])
            if side(b) * side(d) >= 0:
                continue
            zw = [_d_value(rng, scene, "in"), _d_value(rng, scene, rng.choice(["in", beyond])), _d_value(rng, scene, beyond),
                  _d_value(rng, scene, rng.choice(["in", beyond]))]
            uv4 = rng.uniform(-4.0, 4.0, (4, 2)).astype(f32) if t else np.full((4, 2), 0.5, f32)
            i1, i2 = [0, 1, 2], ([2, 3, 0] if k % 2 else [0, 2, 3])
            c1 = _clip_d(xy[i1], [zw[i] for i in i1], 64, 48, scene)
            c2 = _clip_d(xy[i2], [zw[i] for i in i2], 64, 48, scene)
            if not (_d_accept(c1, uv4[i1], 64, 48) and _d_accept(c2, uv4[i2], 64, 48)):
                continue
            t1, t2 = RR.ClippedTri(c1, uv4[i1], 64, 48), RR.ClippedTri(c2, uv4[i2], 64, 48)
            if (t1.coverage() & t2.coverage() & ~(t1.offered() | t2.offered())).any():
                continue  # (w < 0: the halves' images may overlap beyond the shared edge)
            break
        add("pair", c1, uv4[i1], 64, 48, scene, t, both_windings=False)
        add("pair", c2, uv4[i2], 64, 48, scene, t, pair=True, both_windings=False)
        cases[-2].opposite = 1                    # the vertex opposite the shared edge: b of [a, b, c],
        cases[-1].opposite = 1 if k % 2 else 2    # d of [c, d, a] or [a, c, d]
    return cases


_CACHE = {}


def cases(family):
    """the cases of "A32", "A40", "B", "C" or "D", made once"""
    if family not in _CACHE:
        _CACHE[family] = {"A32": lambda: family_a(32, 32, 4101), "A40": lambda: family_a(40, 36, 4102),
                          "B": family_b, "C": family_c, "D": family_d}[family]()
    return _CACHE[family]


_REFS = {}


def reference(case):
    """the reference's result of a case, computed once and shared (callers leave it unchanged)"""
    if case.name not in _REFS:
        _REFS[case.name] = RR.render(case.tris, case.width, case.height, mip_chain_by_rule(case), case.smp, exact=case.exact)
    return _REFS[case.name]


_CHAINS = {}


def set_mip_chain(case, chain):
    """the chain read back from a library; both libraries must return the same one (mip_chain_by_rule holds it to S3)"""
    key = (case.tex, case.mipmapped)
    if key in _CHAINS:
        assert len(chain) == len(_CHAINS[key]) and all(np.array_equal(a, b) for a, b in zip(chain, _CHAINS[key])), \
            f"{key}: this library's mip chain differs from the one read back before"
    else:
        _CHAINS[key] = chain


def mip_chain_by_rule(case):
    """The read-back chain, checked against the rules the reference states for it: floor(log2(max(w, h))) + 1 levels when
    mip-mapped, level extent max(1, w >> l), and every level equal to the chain tests/image_ref.py makes of the texture by
    rule (S3) - so what families C and D sample rests on nothing a library supplied."""
    chain = _CHAINS[(case.tex, case.mipmapped)]
    w, h = TEXTURES[case.tex]
    assert len(chain) == (int(np.floor(np.log2(max(w, h)))) + 1 if case.mipmapped else 1), f"{case.tex}: {len(chain)} levels"
    for l, level in enumerate(chain):
        assert level.shape[:2] == (max(1, h >> l), max(1, w >> l)), f"{case.tex} level {l}: extent {level.shape[:2]}"
    assert np.array_equal(chain[0], texture(case.tex))
    by_rule = IR.mip_chain(texture(case.tex))[:len(chain)]
    for l, (level, want) in enumerate(zip(chain, by_rule)):
        assert np.array_equal(level, want), f"{case.tex} level {l}: the chain read back is not the one the rules give"
    return chain


# ---------------------------------------------------------------- the rig
class Rig:
    """One context per target size; images, samplers and materials are made once."""

    def __init__(self, lib, width, height, attributes=False, color_format=A.COLOR_RGBA16F, instrumented=True, tuning=None):
        self.lib, self.width, self.height, self.attributes = lib, width, height, attributes
        self.color_format, self.instrumented = color_format, instrumented
        self.r = lib.create(width, height, color_format)
        # instrumented by default: the oracle's trace needs it, and HIP passes self-check; off: the timed tile_kernel instances
        self.r.set_option(A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0)
        if tuning is not None:
            self.r.set_option(A.OPT_TUNING, tuning)
        if attributes:
            self.r.enable_attributes(A.ATTR_ALL)
        self.images, self.samplers, self.materials = {}, {}, {}
        vp = np.zeros((4, 4), dtype=f32)
        vp[0][0] = vp[1][1] = 1
        vp[2][2], vp[3][2], vp[2][3] = 0.25, 0.125, 1
        light = dict(ambient=0.0, sun=(0, 1, 0, 1))
        self.scene_projective = A.scene_struct(SC.IDENT, SC.IDENT, vp, [0.0] * 4, light["sun"], (1, 1, 1, 1))
        self.scene_identity = SC.identity_scene(**light)
        nf = np.zeros((4, 4), dtype=f32)
        nf[0][0] = nf[1][1] = 1
        nf[2][2], nf[3][2], nf[2][3] = -0.125, 1.125, 1
        self.scene_nearfar = A.scene_struct(SC.IDENT, SC.IDENT, nf, [0.0] * 4, light["sun"], (1, 1, 1, 1))

    def close(self):
        self.r.close()

    def material(self, case):
        ikey = (case.tex, case.mipmapped)
        if ikey not in self.images:
            img = self.r.create_image(texture(case.tex), mipmapped=case.mipmapped)
            w, h = TEXTURES[case.tex]
            levels = int(np.floor(np.log2(max(w, h)))) + 1 if case.mipmapped else 1
            set_mip_chain(case, [self.r.read_image_level(img, l) for l in range(levels)])
            with np.testing.assert_raises(A.SvrError):
                self.r.read_image_level(img, levels)
            self.images[ikey] = img
        if case.smp not in self.samplers:
            mag, minf, mip, lo, hi = case.smp
            self.samplers[case.smp] = self.r.create_sampler(mag=mag, minf=minf, mip=mip, min_lod=lo, max_lod=hi)
        mkey = ikey + (case.smp,)
        if mkey not in self.materials:
            self.materials[mkey] = self.r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), self.images[ikey], self.samplers[case.smp])
        return self.materials[mkey]

    def prepare(self, case, tris=None, lead=0):
        """the case's triangles (or `tris`, in its scene and material) as one mesh, behind `lead` zero-area triangles inside
        the volume: they draw nothing, and the first real triangle's primitive index is `lead`"""
        still = (0.0, 0.0, 2.0) if case.projective == "nearfar" else (0.0, 0.0, 0.5)
        pos, uvs = [np.tile(np.array(still, f32), (3, 1))] * lead, [np.zeros((3, 2), f32)] * lead
        for clip, uv in (case.tris if tris is None else tris):
            p = clip[:, [0, 1, 3]].copy() if case.projective else clip[:, :3].copy()
            pos.append(p)
            uvs.append(uv)
        verts = SC.make_vertices(np.concatenate(pos), uvs=np.concatenate(uvs))
        mesh = self.r.upload_mesh(np.arange(len(verts), dtype=np.uint32), verts)
        # bounds are caller data; the near/far scene's span w = 1/2 .. 19/2, whose depths straddle [0, 1] (is_visible's test)
        bounds = dict(origin=(0, 0, 5), extents=(1e6, 1e6, 4.5)) if case.projective == "nearfar" else dict(extents=BIG)
        ro = SC.objs([SC.render_object(mesh, self.material(case), 0, len(verts), **bounds)])
        scene = self.scene_nearfar if case.projective == "nearfar" else self.scene_projective if case.projective else self.scene_identity
        return mesh, ro, scene

    def draw(self, case, trace_pixels=()):
        """One pass over a target cleared to zero alpha.  -> covered (alpha written), depth, colour as float32, and either
        the attribute planes (HIP library) or the traces of `trace_pixels` (one more instrumented pass each)."""
        mesh, ro, scene = self.prepare(case)
        r = self.r
        r.trace_pixel(-1, -1)
        r.clear_color((0.0, 0.0, 0.0, 0.0))
        r.draw_geometry(scene, ro)
        codes = r.read_color()
        # "color": the stored values - halves, or the bytes of an RGBA8 target (0 .. 255)
        color = codes.view(np.float16).astype(np.float32) if self.color_format == A.COLOR_RGBA16F else codes.astype(np.float32)
        out = {"covered": color[..., 3] != 0.0, "depth": r.read_depth(), "color": color,
               "fragments": int(r.get_stats().rasterized_fragments) if self.instrumented else None}
        if self.attributes:
            out["bary"], out["uv"], out["albedo"] = (r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_ALBEDO))
        traces = []
        for x, y in trace_pixels:
            r.trace_pixel(int(x), int(y))
            r.draw_geometry(scene, ro)
            traces.append(r.read_trace().copy())
        if traces:
            r.trace_pixel(-1, -1)
            out["traces"] = np.array(traces)
        r.destroy_mesh(mesh)
        return out
