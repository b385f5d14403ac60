"""Seeded cases for tests/raster_ref.py and the rig that draws them through a library of the svr.h ABI.

Every case is one svr_draw_geometry pass: full scissor, identity world matrix, white vertex colour, colour factors 1,
normal and sun (0, 1, 0), ambient 0, sun intensity 1 - so the light term is 1, colour is the texel and the ALBEDO plane is
the fp32 texel.  Family A uses viewproj = identity (clip = position, w = 1).  Families B and C use a viewproj whose
last row takes w from the position's z: position (x, y, w) -> clip (x, y, w/4 + 1/8, w); every product and sum of that
C0/C1 chain is exact for the values used (x, y pass through; w is a multiple of 2^-8 in [1/4, 16]), so the clip
coordinates the reference is handed are the ones the libraries compute."""
import numpy as np

import __graft_entry__ as g
import raster_ref as RR
import scenarios as SC

pkg = g.load_package()
A = pkg.abi
f32 = np.float32
BIG = (1e6, 1e6, 1e6)  # bounds that is_visible never culls


class Case:
    def __init__(self, name, family, width, height, tris, tex="white", mipmapped=False, smp=(0, 0, 0, 0.0, 0.0),
                 projective=True, exact=False, pair=False):
        self.name, self.family, self.width, self.height = name, family, width, height
        self.tris = tris  # [(clip (3, 4) f32, uv (3, 2) f32)]
        self.tex, self.mipmapped, self.smp, self.projective, self.exact, self.pair = tex, mipmapped, smp, projective, exact, pair


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


_CACHE = {}


def cases(family):
    """the cases of "A32", "A40", "B" or "C", made once"""
    if family not in _CACHE:
        _CACHE[family] = {"A32": lambda: family_a(32, 32, 4101), "A40": lambda: family_a(40, 36, 4102),
                          "B": family_b, "C": family_c}[family]()
    return _CACHE[family]


_REFS = {}


def reference(case):
    """the reference's result of a case, computed once and shared (callers leave it unchanged)"""
    if case.name not in _REFS:
        _REFS[case.name] = RR.render(case.tris, case.width, case.height, mip_chain_by_rule(case), case.smp, exact=case.exact)
    return _REFS[case.name]


_CHAINS = {}


def set_mip_chain(case, chain):
    """the chain read back from a library; both libraries must return the same one (mip generation is pinned elsewhere)"""
    key = (case.tex, case.mipmapped)
    if key in _CHAINS:
        assert len(chain) == len(_CHAINS[key]) and all(np.array_equal(a, b) for a, b in zip(chain, _CHAINS[key])), \
            f"{key}: this library's mip chain differs from the one read back before"
    else:
        _CHAINS[key] = chain


def mip_chain_by_rule(case):
    """The read-back chain, checked against the rules the reference states for it: floor(log2(max(w, h))) + 1 levels when
    mip-mapped, level extent max(1, w >> l)."""
    chain = _CHAINS[(case.tex, case.mipmapped)]
    w, h = TEXTURES[case.tex]
    assert len(chain) == (int(np.floor(np.log2(max(w, h)))) + 1 if case.mipmapped else 1), f"{case.tex}: {len(chain)} levels"
    for l, level in enumerate(chain):
        assert level.shape[:2] == (max(1, h >> l), max(1, w >> l)), f"{case.tex} level {l}: extent {level.shape[:2]}"
    assert np.array_equal(chain[0], texture(case.tex))
    return chain


# ---------------------------------------------------------------- the rig
class Rig:
    """One context per target size; images, samplers and materials are made once."""

    def __init__(self, lib, width, height, attributes=False):
        self.lib, self.width, self.height, self.attributes = lib, width, height, attributes
        self.r = lib.create(width, height)
        self.r.set_option(A.OPT_COUNT_FRAGMENTS, 1)  # instrumented: the oracle's trace needs it, and HIP passes self-check
        if attributes:
            self.r.enable_attributes(A.ATTR_ALL)
        self.images, self.samplers, self.materials = {}, {}, {}
        vp = np.zeros((4, 4), dtype=f32)
        vp[0][0] = vp[1][1] = 1
        vp[2][2], vp[3][2], vp[2][3] = 0.25, 0.125, 1
        light = dict(ambient=0.0, sun=(0, 1, 0, 1))
        self.scene_projective = A.scene_struct(SC.IDENT, SC.IDENT, vp, [0.0] * 4, light["sun"], (1, 1, 1, 1))
        self.scene_identity = SC.identity_scene(**light)

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

    def prepare(self, case):
        pos, uvs = [], []
        for clip, uv in case.tris:
            p = clip[:, [0, 1, 3]].copy() if case.projective else clip[:, :3].copy()
            pos.append(p)
            uvs.append(uv)
        verts = SC.make_vertices(np.concatenate(pos), uvs=np.concatenate(uvs))
        mesh = self.r.upload_mesh(np.arange(len(verts), dtype=np.uint32), verts)
        ro = SC.objs([SC.render_object(mesh, self.material(case), 0, len(verts), extents=BIG)])
        return mesh, ro, (self.scene_projective if case.projective else self.scene_identity)

    def draw(self, case, trace_pixels=()):
        """One pass over a target cleared to zero alpha.  -> covered (alpha written), depth, colour as float32, and either
        the attribute planes (HIP library) or the traces of `trace_pixels` (one more instrumented pass each)."""
        mesh, ro, scene = self.prepare(case)
        r = self.r
        r.trace_pixel(-1, -1)
        r.clear_color((0.0, 0.0, 0.0, 0.0))
        r.draw_geometry(scene, ro)
        color = r.read_color().view(np.float16).astype(np.float32)
        out = {"covered": color[..., 3] != 0.0, "depth": r.read_depth(), "color": color}
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
