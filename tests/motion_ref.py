"""Test-side helpers of the camera motion blur pass (include/svr_motion.h): build and run tests/native/motion_ref.cpp, the
scalar restatement of DESIGN C67-C72, the fp64 statements of the velocity (velocity64) and of the gather (motion64) written
from the header's definitions, and the inputs the tests share.  Colour targets travel as uint16 [H, W, 4] arrays of fp16 bit
patterns, depth as float32 [H, W] (bits 0 where nothing was drawn), matrices as glmath's [column][row] arrays."""
import functools
import math

import numpy as np

import __graft_entry__ as g
import native_ref as N
from dof_ref import Camera, plane_over_wall, random_hdr, rolling_dist  # noqa: F401  (the inputs the issue names; re-exported)
from native_ref import SPECIALS, floats, halves, san_bits  # noqa: F401  (re-exported)

GL = g.load_package().glmath
f32 = np.float32
U = 2.0 ** -24
WRONG_VARIANTS = {1: "depth rule reversed", 2: "tap's reach for every tap", 3: "cover without the + 1", 4: "normalised by S",
                  5: "G from the own cell only", 6: "16 taps always", 7: "shutter not halved", 8: "vy negated", 9: "reach from |v|"}

ref_exe = functools.partial(N.build, "motion_ref")


def run_ref(color, depth, reproject, shutter, max_blur, scissor=None, variant=0):
    """motion_ref over a colour target and its depth -> dict(color: uint16 [H, W, 4] after the pass, rgb: uint16 [sh, sw, 3]
    (san'ed), v: uint16 [sh, sw, 2] (the velocity halves, x first), z: float32 [sh, sw], M and G: uint64 [ch, cw], S:
    float32 [sh, sw], the sum of weights)"""
    color = np.ascontiguousarray(color)
    depth = np.ascontiguousarray(depth, dtype=f32)
    assert color.dtype == np.uint16 and color.ndim == 3 and color.shape[2] == 4 and depth.shape == color.shape[:2]
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, variant, 0], np.uint32)
    par = np.concatenate([np.asarray(reproject, f32).reshape(16), np.array([shutter, max_blur], f32)])
    raw = N.run(ref_exe(), hdr.tobytes() + par.tobytes() + color.tobytes() + depth.tobytes())
    n = w * h * 8
    out = np.frombuffer(raw[:n], np.uint16).reshape(h, w, 4).copy()
    cw, ch = (int(v) for v in np.frombuffer(raw[n:n + 8], np.uint32))
    n += 8
    prep = np.frombuffer(raw[n:n + sw * sh * 16], np.uint16).reshape(sh, sw, 8).copy()
    n += sw * sh * 16
    M = np.frombuffer(raw[n:n + cw * ch * 8], np.uint64).reshape(ch, cw).copy()
    n += cw * ch * 8
    G = np.frombuffer(raw[n:n + cw * ch * 8], np.uint64).reshape(ch, cw).copy()
    n += cw * ch * 8
    S = np.frombuffer(raw[n:], f32).reshape(sh, sw).copy()
    z = np.ascontiguousarray(prep[..., 6:8]).view(np.uint32).reshape(sh, sw).view(f32)
    return dict(color=out, rgb=prep[..., :3].copy(), v=prep[..., 4:6].copy(), z=z, M=M, G=G, S=S)


def camera_reproject(w, h, position=(0.0, 0.0, 0.0), yaw=0.0):
    """SvrMotionBlurPass.reproject for this frame's camera at `position` turned by `yaw`, the previous frame's at the origin
    with no yaw, under the project's projection for a w x h target"""
    proj = Camera(w, h).proj
    now = GL.matmul(proj, GL.camera_view(np.array(position, f32), f32(0), f32(yaw)))
    prev = GL.matmul(proj, GL.camera_view(np.zeros(3, f32), f32(0), f32(0)))
    return GL.temporal_reproject(prev, now)


def affine_reproject(ax=0.0, bx=0.0, ay=0.0, by=0.0):
    """an NDC-affine reprojection: q = (xn + ax z + bx, yn + ay z + by, z, 1).  With powers of two for the entries, the
    extents and the depths every product of C67 is exact: a surface with ax z + bx == 0 has velocity exactly 0"""
    m = GL.identity()
    m[2][0], m[3][0], m[2][1], m[3][1] = f32(ax), f32(bx), f32(ay), f32(by)
    return m


# ---------------------------------------------------------------- the fp64 statements, from the definitions
def velocity64(depth, reproject, shutter, max_blur, W, H, origin=(0, 0)):
    """C67 in float64 from the fp32 parameters, before the rounding to halves -> dict(v: float64 [h, w, 2], qw: float64
    [h, w], bound: float64 [h, w, 2], the first-order fp32 error of v by C67's operation count; see tests/test_motion_ref.py)"""
    m = np.asarray(reproject, f32).astype(np.float64)  # [column][row]
    h, w = depth.shape
    y, x = np.mgrid[0:h, 0:w]
    fx, fy = x + origin[0] + 0.5, y + origin[1] + 0.5
    xn, yn = fx * (2.0 / W) - 1.0, fy * (2.0 / H) - 1.0
    z = depth.astype(np.float64)
    q = [m[0][r] * xn + m[1][r] * yn + m[2][r] * z + m[3][r] for r in range(4)]
    # the magnitude the C0 chain's roundings are relative to: the sum of the terms' sizes (a bound of every partial sum)
    qa = [np.abs(m[0][r] * xn) + np.abs(m[1][r] * yn) + np.abs(m[2][r] * z) + np.abs(m[3][r]) for r in range(4)]
    hs = 0.5 * float(f32(shutter))
    mb = float(f32(max_blur))
    half = (W / 2.0, H / 2.0)
    v, bound = np.zeros((h, w, 2)), np.zeros((h, w, 2))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        aw = np.abs(q[3])
        for a, f in enumerate((fx, fy)):
            n = q[a] / q[3]
            hh = n * half[a] + half[a]
            v[..., a] = (f - hh) * hs
            # xn, yn: the quotient 2 / extent, the fma: 2 u (|f| two_over + 1) each, carried through their columns;
            d_in = 2 * U * ((np.abs(fx) * (2.0 / W) + 1) * np.abs(m[0][a]) + (np.abs(fy) * (2.0 / H) + 1) * np.abs(m[1][a]))
            d_inw = 2 * U * ((np.abs(fx) * (2.0 / W) + 1) * np.abs(m[0][3]) + (np.abs(fy) * (2.0 / H) + 1) * np.abs(m[1][3]))
            # the chain: a product and three fmas, 4 u of the terms' sizes
            dq, dw = 4 * U * qa[a] + d_in, 4 * U * qa[3] + d_inw
            # r = 1 / q.w (u), q r (u): n's error; the fma (u of its result's size, at most |n| half + half); the difference
            # (u); the product with hs (u)
            dn = dq / aw + np.abs(n) * dw / aw + 2 * U * np.abs(n)
            dh = dn * half[a] + U * (np.abs(n) * half[a] + half[a])
            bound[..., a] = (dh + U * np.abs(f - hh)) * hs + U * np.abs(v[..., a])
        dead = ~(q[3] > 0) | ~np.isfinite(v).all(-1)
        v[dead] = 0.0
        bound[dead] = 0.0
        l = np.hypot(v[..., 0], v[..., 1])
        over = l > mb
        # clamped: l carries the components' errors (|dl| <= |dvx| + |dvy|) and three roundings (the product, the fma, the
        # root: at most 2 u l), k = max_blur / l one and the product one: 4 u max_blur beside the components' own errors
        # scaled by k and the direction's, |v k| dl / l.  A pixel whose l lies within 2^-16 of max_blur may take the other
        # branch in fp32: there k is 1 within those same errors, so it gets the clamped allowance too
        near = l > mb * (1.0 - 2.0 ** -16)
        safe_l = np.where(near, l, 1.0)
        k = np.where(over, mb / safe_l, 1.0)
        clamped = bound * k[..., None] + np.abs(v * k[..., None]) * (bound.sum(-1) / safe_l)[..., None] + 4 * U * mb
        bound = np.where(near[..., None], clamped, bound)
        v = v * k[..., None]
    return dict(v=v, qw=q[3], bound=bound)


def _round24(n):
    """non-negative int64 -> the nearest integer with 24 significant bits, ties to even (an fp32 rounding, on integers)"""
    n = np.asarray(n, np.int64)
    bl = np.zeros(n.shape, np.int64)
    t = n.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = t >= (np.int64(1) << s)
        bl += np.where(big, s, 0)
        t = np.where(big, t >> s, t)
    bl += (t > 0)
    shift = np.maximum(bl - 24, 0)
    q = n >> shift
    rem = n - (q << shift)
    half = np.where(shift > 0, np.int64(1) << np.maximum(shift - 1, 0), 0)
    up = (shift > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    return (q + up) << shift


def keys64(v_bits):
    """C69's key of every texel from the velocity halves [h, w, 2], through exact integers: len2 = vx^2 + vy^2 in units of
    2^-48 (at most 2^57), rounded once to 24 bits"""
    iv = np.rint(floats(v_bits).astype(np.float64) * 2.0 ** 24).astype(np.int64)
    len2 = _round24(iv[..., 0] * iv[..., 0] + iv[..., 1] * iv[..., 1]).astype(np.float64) * 2.0 ** -48  # exact: 24 bits
    hi = len2.astype(f32).view(np.uint32).astype(np.uint64)
    return (hi << np.uint64(32)) | (v_bits[..., 0].astype(np.uint64) << np.uint64(16)) | v_bits[..., 1].astype(np.uint64)


def cells64(v_bits, max_blur):
    """C69 -> (M, G), uint64 [ch, cw]"""
    h, w = v_bits.shape[:2]
    ch, cw = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ch * 8, cw * 8), np.uint64)
    pad[:h, :w] = keys64(v_bits)
    M = pad.reshape(ch, 8, cw, 8).max(axis=(1, 3))
    Rc = (int(math.ceil(float(f32(max_blur)))) + 7) // 8
    G = np.zeros_like(M)
    for cy in range(ch):
        for cx in range(cw):
            ys = np.clip(np.arange(cy - Rc, cy + Rc + 1), 0, ch - 1)
            xs = np.clip(np.arange(cx - Rc, cx + Rc + 1), 0, cw - 1)
            G[cy, cx] = M[np.ix_(ys, xs)].max()
    return M, G


def motion64(rgb, v_bits, z, max_blur):
    """The gather in float64 over a prepared image (rgb: uint16 [h, w, 3], san'ed; v_bits: uint16 [h, w, 2]; z: float32
    [h, w]), written from include/svr_motion.h's definitions.  Returns dict(out: float64 [h, w, 3] before the store's
    rounding, bound: float64 [h, w, 3], the first-order fp32 error of out by the operation counts of C71 and C72 (see
    tests/test_motion_ref.py), n: int [h, w], the tap count (0 in a cell that copies), S: float64 [h, w], M, G)."""
    h, w = z.shape
    I = floats(rgb).astype(np.float64)
    v = floats(v_bits).astype(np.float64)
    zz = z.astype(np.float64)
    M, G = cells64(v_bits, max_blur)
    Gp = np.repeat(np.repeat(G, 8, axis=0), 8, axis=1)[:h, :w]
    L2 = (Gp >> np.uint64(32)).astype(np.uint32).view(f32).astype(np.float64)
    gx = floats(((Gp >> np.uint64(16)) & np.uint64(0xffff)).astype(np.uint16)).astype(np.float64)
    gy = floats((Gp & np.uint64(0xffff)).astype(np.uint16)).astype(np.float64)
    live_cell = L2 >= 0.25
    n = np.where(live_cell, np.where(L2 > 64.0, 32, 16), 0)
    gl = np.sqrt(np.where(live_cell, L2, 1.0))

    def e_of(vv):  # a texel's reach along the pixel's cell's dominant direction
        return np.abs(vv[..., 0] * gx + vv[..., 1] * gy) / gl

    ep = e_of(v)
    y, x = np.mgrid[0:h, 0:w]
    acc, S = np.zeros((h, w, 3)), np.zeros((h, w))
    e_acc, e_S, m = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    nn = np.maximum(n, 1).astype(np.float64)
    for k in range(32):
        s = (2 * (k >> 1) + 1) / nn * (-1.0 if k & 1 else 1.0)
        dx, dy = np.rint(gx * s).astype(int), np.rint(gy * s).astype(int)
        live = (k < n) & ((dx != 0) | (dy != 0))
        tx, ty = np.clip(x + dx, 0, w - 1), np.clip(y + dy, 0, h - 1)
        D = np.sqrt((dx * dx + dy * dy).astype(np.float64))
        with np.errstate(invalid="ignore"):
            e = np.where(zz[ty, tx] < zz, ep, e_of(v[ty, tx]))
        wk = np.where(live, np.clip(e - D + 1.0, 0.0, 1.0), 0.0)
        Ik = I[ty, tx]
        acc += wk[..., None] * Ik
        S += wk
        # fp32: e carries the fma (the product of two halves is exact), the root, the reciprocal and the product, 4 u e; D one
        # root, u D; the difference rounds once, at most u (e + D), and the + 1 once more, at most u where it matters (the sum
        # lies in [0, 1]); sat does not widen an error
        dw = np.where(live, U * (5.0 * e + 2.0 * D + 1.0), 0.0)
        e_acc += dw[..., None] * Ik
        e_S += dw
        m += live
    rest = n - S
    total = acc + rest[..., None] * I
    # ... every fma and every addition of the running sums rounds once, at most the final sum's size each (no term is
    # negative); n - S rounds once, at most u n; the last fma once more; the scaling by 1 / n is exact
    e_total = e_acc + (e_S + m * U * S + U * n)[..., None] * I + ((m + 1) * U)[..., None] * total
    out = np.where(live_cell[..., None], total / nn[..., None], I)
    bound = np.where(live_cell[..., None], e_total / nn[..., None], 0.0)
    return dict(out=out, bound=bound, n=n, S=S, M=M, G=G)
