"""Test-side helpers of the fog pass (include/svr_fog.h): build and run tests/native/fog_ref.cpp, the scalar restatement of
DESIGN C55-C60, the fp64 statement of the same march written from the definitions (march64), and the inputs the tests
share.  Colour targets travel as uint16 [H, W, 4] arrays of fp16 bit patterns, depth as float32 [H, W] (reversed-Z: 1 at
the near plane, bits 0 where nothing was drawn), a shadow map as float32 [Hs, Ws].  Matrices are 4 x 4 numpy arrays in
the mathematical convention (M @ column vector); colmajor() gives the 16 floats the C structs hold."""
import functools
import math

import numpy as np

import native_ref as N
from native_ref import SPECIALS, floats, halves  # noqa: F401  (re-exported)

f32 = np.float32
WRONG_VARIANTS = {1: "T updated before S", 2: "dither dropped", 3: "sample at the step's start", 4: "plain bilinear upsample",
                  5: "bias sign flipped", 6: "height measured from the camera", 7: "g negated",
                  8: "block marched to its nearest pixel", 9: "tap clamp off by one"}
DEFAULTS = dict(density=0.05, height_falloff=0.0, height_base=0.0, max_distance=60.0, steps=16, fog_color=(0.5, 0.6, 0.7),
                sun_dir=(0.3, 0.8, 0.5, 0.0), sun_color=(0.0, 0.0, 0.0), anisotropy=0.0, shadow_viewproj=None, shadow_bias=0.0,
                edge_sharpness=1.0, frame_index=0)


ref_exe = functools.partial(N.build, "fog_ref")


def colmajor(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16).astype(f32))


def run_ref(color, depth, inv_viewproj, camera, scissor=None, shadow=None, variant=0, pin_o=None, **kw):
    """fog_ref over a colour target and its depth -> dict(color: uint16 [H, W, 4] after the pass, st: float32 [gh, gw, 4]
    (S.rgb, T per block), t_end: float32 [gh, gw]).  inv_viewproj and kw["shadow_viewproj"]: 16 floats, column-major"""
    p = dict(DEFAULTS, **kw)
    color = np.ascontiguousarray(color)
    depth = np.ascontiguousarray(depth, dtype=f32)
    assert color.dtype == np.uint16 and color.ndim == 3 and color.shape[2] == 4 and depth.shape == color.shape[:2]
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    hs, ws = shadow.shape if shadow is not None else (0, 0)
    hdr = np.array([w, h, sx, sy, sw, sh, p["steps"], p["frame_index"] & 0xffffffff, ws, hs, variant, 0 if pin_o is None else 1], np.uint32)
    svp = p["shadow_viewproj"] if shadow is not None else np.zeros(16, f32)
    par = np.concatenate([np.asarray(inv_viewproj, f32).reshape(16), np.asarray(camera, f32).reshape(3),
                          [p["density"], p["height_falloff"], p["height_base"], p["max_distance"]], np.asarray(p["fog_color"], f32)[:3],
                          [p["anisotropy"]], (list(p["sun_dir"]) + [0.0])[:4], np.asarray(p["sun_color"], f32)[:3], [p["edge_sharpness"]],
                          np.asarray(svp, f32).reshape(16), [p["shadow_bias"], 0.0 if pin_o is None else pin_o]]).astype(f32)
    assert par.size == 53
    smap = b"" if shadow is None else np.ascontiguousarray(shadow, dtype=f32).tobytes()
    raw = N.run(ref_exe(), hdr.tobytes() + par.tobytes() + color.tobytes() + depth.tobytes() + smap)
    n = w * h * 8
    out = np.frombuffer(raw[:n], np.uint16).reshape(h, w, 4).copy()
    gw, gh = np.frombuffer(raw[n:n + 8], np.uint32)
    st = np.frombuffer(raw[n + 8:n + 8 + gw * gh * 16], f32).reshape(gh, gw, 4).copy()
    te = np.frombuffer(raw[n + 8 + gw * gh * 16:], f32).reshape(gh, gw).copy()
    return dict(color=out, st=st, t_end=te)


def random_hdr(w, h, seed, specials=False):
    """a seeded RGBA16F target, uint16 [h, w, 4]: values from 0 to about 8; with specials, NaN, +-inf, negative halves, -0 and
    subnormals sprinkled over it"""
    rng = np.random.default_rng(seed)
    out = halves(rng.uniform(0.0, 2.0, (h, w, 4)) ** 3)
    if specials:
        hit = rng.random((h, w, 4)) < 0.08
        out[hit] = SPECIALS[rng.integers(0, SPECIALS.size, int(hit.sum()))]
    return out


# ---------------------------------------------------------------- a camera and synthetic depth
def perspective(fov_y, aspect, near):
    """reversed-Z, infinite far plane, looking down -z: depth = near / distance along the axis (1 at the near plane)"""
    f = 1.0 / math.tan(0.5 * fov_y)
    return np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, 0, near], [0, 0, -1, 0]], np.float64)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = right, upv, -fwd
    V[:3, 3] = -V[:3, :3] @ eye
    return V


class Camera:
    """eye, a view-projection (float32 values, kept as float64) and its inverse, as the pass takes them"""

    def __init__(self, w, h, eye=(0.5, 1.0, 1.5), target=(0.0, 0.5, -10.0), fov_y=1.0, near=0.5):
        self.w, self.h, self.near = w, h, near
        self.eye = np.asarray(eye, f32)
        self.viewproj = perspective(fov_y, w / h, near) @ look_at(self.eye.astype(np.float64), target)
        self.inv = colmajor(np.linalg.inv(self.viewproj))

    def max_dir_y(self):
        """the largest |y| of a unit ray through the image, from its four corners"""
        Minv = np.linalg.inv(self.viewproj)
        out = 0.0
        for xn in (-1.0, 1.0):
            for yn in (-1.0, 1.0):
                q = Minv @ np.array([xn, yn, 1.0, 1.0])
                d = q[:3] / q[3] - self.eye.astype(np.float64)
                out = max(out, abs(d[1]) / np.linalg.norm(d))
        return out

    def depth_of(self, axial):
        """the depth texels of surfaces `axial` world units in front of the camera along its axis; 0 where axial is inf"""
        with np.errstate(divide="ignore"):
            return np.where(np.isfinite(axial), self.near / np.asarray(axial, np.float64), 0.0).astype(f32)


def split_wall(w, h, near_d=2.0, far_d=40.0):
    """axial distances [h, w]: the left half a near wall, the right half a far one"""
    d = np.full((h, w), far_d)
    d[:, :w // 2] = near_d
    return d


def rolling_depth(w, h, seed, lo=3.0, hi=30.0, holes=0.1):
    """smooth seeded axial distances in [lo, hi] with a step across the middle row, and a share of cleared pixels (inf)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = lo + (hi - lo) * (0.5 + 0.25 * np.sin(x * 0.37 + rng.uniform(0, 6)) + 0.25 * np.cos(y * 0.23 + rng.uniform(0, 6)))
    d[h // 2:] *= 0.6
    d[rng.random((h, w)) < holes] = np.inf
    return d


def ortho_light(center=(0.0, 0.0, -12.0), half=16.0, height=40.0):
    """an orthographic sun camera looking straight down on a (2 half)^2 square around center, reversed-Z over `height` units
    below y = center.y + height / 2: clip w is 1 everywhere.  Returns (viewproj float64 4x4, its direction towards the sun)"""
    cx, cy, cz = center
    top = cy + 0.5 * height
    # x_ndc = (x - cx) / half, y_ndc = (z - cz) / half, depth = 1 - (top - y) / height  (nearer the light: larger)
    M = np.array([[1 / half, 0, 0, -cx / half], [0, 0, 1 / half, -cz / half], [0, 1 / height, 0, 1 - top / height], [0, 0, 0, 1]], np.float64)
    return M, (0.0, 1.0, 0.0, 0.0)


def slab_map(n, M_light, seed, lo_y=2.0, hi_y=8.0, open_share=0.5):
    """a coarse n x n map under ortho_light: each texel either open (depth 0: nothing above the ground) or an occluder slab at
    a seeded height in [lo_y, hi_y]; float32 [n, n]"""
    rng = np.random.default_rng(seed)
    ys = rng.uniform(lo_y, hi_y, (n, n))
    depth = M_light[2, 1] * ys + M_light[2, 3]
    depth[rng.random((n, n)) < open_share] = 0.0
    return depth.astype(f32)


def spot_light(eye=(0.0, 4.0, -6.0), fov=2.0, near=0.5):
    """a perspective light looking straight down from eye: clip w is the distance below it, so a sample above the light has
    w < 0 and C18's `q.w > 0` decides.  Returns (viewproj float64 4x4, its direction towards the light)"""
    return perspective(fov, 1.0, near) @ look_at(eye, (eye[0], 0.0, eye[2]), up=(0.0, 0.0, -1.0)), (0.0, 1.0, 0.0, 0.0)


def spot_map(n, seed, eye_y=4.0, near=0.5, lo_y=1.0, hi_y=3.5, open_share=0.5):
    """a coarse n x n map under spot_light: each texel either open (depth 0) or an occluder at a seeded height in
    [lo_y, hi_y], reversed-Z: near / (eye_y - y); float32 [n, n]"""
    rng = np.random.default_rng(seed)
    depth = near / (eye_y - rng.uniform(lo_y, hi_y, (n, n)))
    depth[rng.random((n, n)) < open_share] = 0.0
    return depth.astype(f32)


# ---------------------------------------------------------------- the fp64 statement, from the definitions
def fog_hash(bx, by, frame):
    M = 0xffffffff
    h = ((bx * 0x9E3779B1) ^ (by * 0x85EBCA77) ^ (frame * 0xC2B2AE3D)) & M
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M
    h ^= h >> 15
    h = (h * 0x846CA68B) & M
    h ^= h >> 16
    return h


def march64(depth, inv_viewproj, camera, scissor=None, shadow=None, pin_o=None, **kw):
    """The half-resolution march in float64, written from include/svr_fog.h's definitions: exp() for the extinction and the
    transmittance, no polynomial, no fma.  Returns dict(S [gh, gw, 3], T [gh, gw], t_end [gh, gw], edge [gh, gw]: the
    smallest distance of any of the ray's samples to a texel edge or the map's border, in texels (inf without a map),
    gap [gh, gw]: the smallest |sz + bias - map| of its samples inside the map (inf without))."""
    p = dict(DEFAULTS, **kw)
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    Minv = np.asarray(inv_viewproj, f32).astype(np.float64).reshape(4, 4).T
    cam = np.asarray(camera, f32).astype(np.float64)
    maxd, steps = float(f32(p["max_distance"])), int(p["steps"])
    density, falloff, base = (float(f32(p[k])) for k in ("density", "height_falloff", "height_base"))
    fog = np.asarray(p["fog_color"], f32).astype(np.float64)[:3]
    sun_c = np.asarray(p["sun_color"], f32).astype(np.float64)[:3]
    L = np.asarray(p["sun_dir"], f32).astype(np.float64)[:3]
    L = L / np.linalg.norm(L) if np.linalg.norm(L) > 0 else np.zeros(3)
    gani = float(f32(p["anisotropy"]))
    bias = float(f32(p["shadow_bias"]))
    if shadow is not None:
        Ms = np.asarray(p["shadow_viewproj"], f32).astype(np.float64).reshape(4, 4).T
        hs, ws = shadow.shape
        smap = shadow.astype(np.float64)

    def unproject(px, py, z):
        q = Minv @ np.array([(px) * 2.0 / w - 1.0, (py) * 2.0 / h - 1.0, z, 1.0])
        return q[:3] / q[3]

    def t_pixel(x, y):
        z = depth[y, x]
        if np.asarray(z, f32).view(np.uint32) == 0:
            return maxd
        return min(float(np.linalg.norm(unproject(x + 0.5, y + 0.5, float(z)) - cam)), maxd)

    gw, gh = (sw + 1) // 2, (sh + 1) // 2
    S, T, TE = np.zeros((gh, gw, 3)), np.ones((gh, gw)), np.zeros((gh, gw))
    EDGE, GAP = np.full((gh, gw), np.inf), np.full((gh, gw), np.inf)
    for by in range(gh):
        for bx in range(gw):
            xs = [sx + 2 * bx + i for i in (0, 1) if 2 * bx + i < sw]
            ys = [sy + 2 * by + i for i in (0, 1) if 2 * by + i < sh]
            t_end = max(t_pixel(x, y) for y in ys for x in xs)
            v = unproject(sx + 2 * bx + 1.0, sy + 2 * by + 1.0, 1.0) - cam
            d = v / np.linalg.norm(v)
            delta = t_end / steps
            o = (fog_hash(bx, by, p["frame_index"] & 0xffffffff) >> 24) / 256.0 if pin_o is None else float(pin_o)
            c = float(d @ L)
            x = 1.0 + gani * gani - 2.0 * gani * c
            ph = (1.0 - gani * gani) / (4.0 * math.pi * x * math.sqrt(x))
            s, tr = np.zeros(3), 1.0
            for i in range(steps):
                ti = (i + o) * delta
                pos = cam + ti * d
                sigma = density * math.exp(-falloff * (pos[1] - base))
                a = math.exp(-sigma * delta)
                vis = 1.0
                if shadow is not None:
                    q = Ms @ np.append(pos, 1.0)
                    if q[3] > 0:
                        u, vv, sz = (q[0] / q[3] * 0.5 + 0.5) * ws, (q[1] / q[3] * 0.5 + 0.5) * hs, q[2] / q[3]
                        fx, fy = math.floor(u), math.floor(vv)
                        EDGE[by, bx] = min(EDGE[by, bx], abs(u - round(u)), abs(vv - round(vv)))
                        if 0 <= fx < ws and 0 <= fy < hs:
                            GAP[by, bx] = min(GAP[by, bx], abs(sz + bias - smap[fy, fx]))
                            if sz + bias < smap[fy, fx]:
                                vis = 0.0
                s = s + tr * (1.0 - a) * (fog + sun_c * (vis * ph))
                tr = tr * a
            S[by, bx], T[by, bx], TE[by, bx] = s, tr, t_end
    return dict(S=S, T=T, t_end=TE, edge=EDGE, gap=GAP)


def sample_points64(depth, inv_viewproj, camera, steps, frame_index, max_distance):
    """float64 [gh, gw, steps, 3]: the world positions the march of the whole target samples, by march64's definitions
    (the inputs must hold no NaN)"""
    h, w = depth.shape
    Minv = np.asarray(inv_viewproj, f32).astype(np.float64).reshape(4, 4).T
    cam = np.asarray(camera, f32).astype(np.float64)
    maxd = float(f32(max_distance))

    def unproject(px, py, z):
        q = np.stack([px * 2.0 / w - 1.0, py * 2.0 / h - 1.0, z, np.ones_like(z)], -1) @ Minv.T
        return q[..., :3] / q[..., 3:]

    gw, gh = (w + 1) // 2, (h + 1) // 2
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(np.linalg.norm(unproject(x + 0.5, y + 0.5, depth.astype(np.float64)) - cam, axis=-1), maxd)
    t[depth.view(np.uint32) == 0] = maxd
    padded = np.full((2 * gh, 2 * gw), -np.inf)
    padded[:h, :w] = t
    t_end = padded.reshape(gh, 2, gw, 2).max(axis=(1, 3))
    by, bx = np.mgrid[0:gh, 0:gw]
    v = unproject(2.0 * bx + 1.0, 2.0 * by + 1.0, np.ones((gh, gw))) - cam
    d = v / np.linalg.norm(v, axis=-1, keepdims=True)
    o = np.array([[(fog_hash(int(b), int(a), frame_index & 0xffffffff) >> 24) / 256.0 for b in range(gw)] for a in range(gh)])
    ti = (np.arange(steps)[None, None, :] + o[..., None]) * (t_end / steps)[..., None]
    return cam + ti[..., None] * d[:, :, None, :]
