"""Test-side helpers of the depth of field pass (include/svr_dof.h): build and run tests/native/dof_ref.cpp, the scalar
restatement of DESIGN C61-C66, the fp64 statement of the same gather written from the definitions (dof64), the tap table
from its formula, and the inputs the tests share.  Colour targets travel as uint16 [H, W, 4] arrays of fp16 bit patterns,
depth as float32 [H, W] (bits 0 where nothing was drawn)."""
import functools
import math
import subprocess

import numpy as np

import __graft_entry__ as g
import native_ref as N
from native_ref import SPECIALS, floats, halves, san_bits  # noqa: F401  (re-exported)

GL = g.load_package().glmath
f32 = np.float32
U = 2.0 ** -24
WRONG_VARIANTS = {1: "the sign of c flipped", 2: "min rule dropped", 3: "cover without the + 1", 4: "1 / e instead of 1 / e^2",
                  5: "centre tap left out", 6: "zero-offset taps counted", 7: "cell reach one cell short", 8: "M over the tile",
                  9: "tap clamp off by one", 10: "dist from the clamped offsets", 11: "even ring not turned", 12: "r clamped from above only"}


ref_exe = functools.partial(N.build, "dof_ref")


def run_ref(color, depth, terms, focus_distance, blur_scale, max_radius, scissor=None, variant=0):
    """dof_ref over a colour target and its depth -> dict(color: uint16 [H, W, 4] after the pass, prepared: uint16
    [sh, sw, 4] (san(rgb) and c as halves), M and g: float32 [ch, cw]).  terms: (inv_z_scale, inv_z_bias)"""
    color = np.ascontiguousarray(color)
    depth = np.ascontiguousarray(depth, dtype=f32)
    assert color.dtype == np.uint16 and color.ndim == 3 and color.shape[2] == 4 and depth.shape == color.shape[:2]
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, variant, 0], np.uint32)
    par = np.array([terms[0], terms[1], focus_distance, blur_scale, max_radius], f32)
    raw = N.run(ref_exe(), hdr.tobytes() + par.tobytes() + color.tobytes() + depth.tobytes())
    n = w * h * 8
    out = np.frombuffer(raw[:n], np.uint16).reshape(h, w, 4).copy()
    cw, ch = (int(v) for v in np.frombuffer(raw[n:n + 8], np.uint32))
    n += 8
    prep = np.frombuffer(raw[n:n + sw * sh * 8], np.uint16).reshape(sh, sw, 4).copy()
    n += sw * sh * 8
    M = np.frombuffer(raw[n:n + cw * ch * 4], f32).reshape(ch, cw).copy()
    G = np.frombuffer(raw[n + cw * ch * 4:], f32).reshape(ch, cw).copy()
    return dict(color=out, prepared=prep, M=M, g=G)


def ref_taps():
    """the table dof_ref.cpp holds, as uint32 bit patterns [49, 2]"""
    out = subprocess.run([ref_exe(), "--taps"], check=True, stdout=subprocess.PIPE, text=True).stdout
    return np.array([[int(v, 16) for v in line.split()] for line in out.splitlines()], np.uint32)


def tap_table():
    """C64 from its formula: float32 [49, 2], computed in float64 and rounded once"""
    t = [(0.0, 0.0)]
    for j in (1, 2, 3):
        for i in range(8 * j):
            a = (2.0 * math.pi) * (i + (0.5 if j % 2 == 0 else 0.0)) / (8 * j)
            x, y = (j / 3.0) * math.cos(a), (j / 3.0) * math.sin(a)
            t.append((0.0 if abs(x) < 2.0 ** -40 else x, 0.0 if abs(y) < 2.0 ** -40 else y))
    return np.array(t, np.float64).astype(f32)


def random_hdr(w, h, seed, specials=False):
    """a seeded RGBA16F target, uint16 [h, w, 4]: values from 0 to about 8; with specials, NaN, +-inf, negative halves, -0 and
    subnormals sprinkled over it"""
    rng = np.random.default_rng(seed)
    out = halves(rng.uniform(0.0, 2.0, (h, w, 4)) ** 3)
    if specials:
        hit = rng.random((h, w, 4)) < 0.08
        out[hit] = SPECIALS[rng.integers(0, SPECIALS.size, int(hit.sum()))]
    return out


# ---------------------------------------------------------------- cameras and synthetic depth
class Camera:
    """the project's projection (glmath.scene_data's: 70 degrees, reversed Z between 10000 and 0.1) for a w x h target: the
    depth terms of the pass, and the depth texels of surfaces at given view distances"""

    def __init__(self, w, h):
        self.proj = GL.perspective_rh_zo(GL.radians(70.0), f32(w) / f32(h), 10000.0, 0.1)
        self.proj[1][1] *= f32(-1)
        self.terms = tuple(float(v) for v in GL.dof_depth_terms(self.proj))

    def depth_of(self, dist):
        """depth = (proj[2][2] z + proj[3][2]) / -z at z = -dist, in double, rounded once; bits 0 where dist is inf"""
        a, b = float(self.proj[2][2]), float(self.proj[3][2])
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.isfinite(dist), (b - a * np.asarray(dist, np.float64)) / np.asarray(dist, np.float64), 0.0).astype(f32)


class UnitCamera:
    """depth = 1 / view distance, terms (1, 0): with a power of two as the focus distance, a surface at it has the radius 0
    exactly (fma(-focus, 1 / focus, 1) == 0), which the consequences of C66 need"""
    terms = (1.0, 0.0)

    @staticmethod
    def depth_of(dist):
        with np.errstate(divide="ignore"):
            return np.where(np.isfinite(dist), 1.0 / np.asarray(dist, np.float64), 0.0).astype(f32)


def rolling_dist(w, h, seed, lo=3.0, hi=30.0, holes=0.1):
    """smooth seeded view distances in [lo, hi] with a step across the middle row, and a share of cleared pixels (inf)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = lo + (hi - lo) * (0.5 + 0.25 * np.sin(x * 0.37 + rng.uniform(0, 6)) + 0.25 * np.cos(y * 0.23 + rng.uniform(0, 6)))
    d[h // 2:] *= 0.6
    d[rng.random((h, w)) < holes] = np.inf
    return d


def plane_over_wall(w, h, edge, near_d, far_d):
    """view distances [h, w]: columns left of `edge` a near plane, the rest a far wall"""
    d = np.full((h, w), float(far_d))
    d[:, :edge] = near_d
    return d


def radius64(depth, terms, focus_distance, blur_scale, max_radius):
    """C61 in float64 from the fp32 parameters, before the rounding to a half"""
    s, b, zf, k, m = (float(f32(v)) for v in (terms[0], terms[1], focus_distance, blur_scale, max_radius))
    with np.errstate(invalid="ignore", over="ignore"):
        r = k * (1.0 - zf * (depth.astype(np.float64) * s + b))
    return np.clip(np.where(np.isnan(r), 0.0, r), -m, m)


# ---------------------------------------------------------------- the fp64 statement, from the definitions
def dof64(prepared, max_radius, taps=None):
    """The gather in float64 over a prepared image (uint16 [h, w, 4]: the san'ed RGB halves and the half-quantised radii c),
    written from include/svr_dof.h's definitions.  Returns dict(out: float64 [h, w, 3] before the store's rounding, tie:
    bool [h, w], True where a tap's u_k * g lies within 2^-18 of a half-integer, bound: float64 [h, w, 3], the first-order
    fp32 error of out by the operation counts of C65 and C66 (see tests/test_dof_ref.py), g: float64 [ch, cw])."""
    taps = (tap_table() if taps is None else taps).astype(np.float64)
    h, w = prepared.shape[:2]
    I = floats(prepared[..., :3]).astype(np.float64)
    c = floats(prepared[..., 3]).astype(np.float64)
    ch, cw = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ch * 8, cw * 8))
    pad[:h, :w] = np.abs(c)
    M = pad.reshape(ch, 8, cw, 8).max(axis=(1, 3))
    R = int(math.ceil(float(f32(max_radius))))
    Rc = (R + 7) // 8
    G = np.zeros_like(M)
    for cy in range(ch):
        for cx in range(cw):
            ys = np.clip(np.arange(cy - Rc, cy + Rc + 1), 0, ch - 1)
            xs = np.clip(np.arange(cx - Rc, cx + Rc + 1), 0, cw - 1)
            G[cy, cx] = M[np.ix_(ys, xs)].max()
    gp = np.repeat(np.repeat(G, 8, axis=0), 8, axis=1)[:h, :w]
    y, x = np.mgrid[0:h, 0:w]
    acc, W = np.zeros((h, w, 3)), np.zeros((h, w))
    e_acc, e_W, n = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    tie = np.zeros((h, w), bool)
    acp = np.abs(c)
    for k in range(taps.shape[0]):
        px, py = taps[k, 0] * gp, taps[k, 1] * gp
        for v in (px, py):
            tie |= np.abs(np.abs(v - np.floor(v)) - 0.5) < 2.0 ** -18
        dx, dy = np.rint(px).astype(int), np.rint(py).astype(int)
        live = np.ones((h, w), bool) if k == 0 else (dx != 0) | (dy != 0)
        tx, ty = np.clip(x + dx, 0, w - 1), np.clip(y + dy, 0, h - 1)
        dist = np.sqrt((dx * dx + dy * dy).astype(np.float64))
        ck = c[ty, tx]
        ack = np.abs(ck)
        e = np.where(ck > c, np.minimum(ack, acp), ack)
        den = np.maximum(e * e, 1.0)
        wk = np.where(live, np.clip(e - dist + 1.0, 0.0, 1.0) / den, 0.0)
        Ik = I[ty, tx]
        acc += wk[..., None] * Ik
        W += wk
        # fp32: the root, the difference and the sum each round once (u of their own size), sat does not widen an error,
        # e * e is exact (22 bits), the quotient rounds once
        dw = np.where(live, U * (2.0 * dist + e + 1.0) / den + U * wk, 0.0)
        e_acc += dw[..., None] * Ik
        e_W += dw
        n += live
    # ... and every fma and every addition of the running sums rounds once, at most the sum's final size each
    e_acc += (n * U)[..., None] * acc
    e_W += n * U * W
    with np.errstate(invalid="ignore", divide="ignore"):
        out = acc / W[..., None]
        bound = (e_acc + out * e_W[..., None]) / W[..., None] + U * out
    return dict(out=np.clip(out, 0.0, 65504.0), tie=tie, bound=bound, g=G)
