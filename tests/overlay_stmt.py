"""An independent statement of the UI overlay pass (include/svr_overlay.h) in Python; not a translation of
tests/native/overlay_ref.cpp.  Positions are snapped to exact rationals and coverage is decided on them with Python
integers and fractions, in geometric words: a pixel centre strictly inside the triangle is covered; one exactly on an edge
is covered iff that edge is a top edge (horizontal, the triangle below it) or a left edge (the triangle to its right).
Interpolation, filtering and blending run in float64; only the store after every layer is the contract's UNORM8."""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32


def snapped(pos, display_pos, scale):
    """C43 -> Fraction in pixels, or None for a non-finite position"""
    x = (f32(pos) - f32(display_pos)) * f32(scale)  # the contract's two fp32 operations
    if not np.isfinite(x):
        return None
    with np.errstate(over="ignore"):
        big = f32(x) * f32(256.0)
    n = 2 ** 23 if big >= 2.0 ** 23 else (-2 ** 23 if big <= -2.0 ** 23 else round(Fraction(float(x)) * 256))  # round(): ties to even
    return Fraction(n, 256)


def clip_box(clip, display_pos, scale, width, height):
    """C45 -> (x0, y0, x1, y1) in whole pixels, or None for a skipped command"""
    box = []
    for k, extent in ((0, width), (1, height)):
        cmin = (f32(clip[k]) - f32(display_pos[k])) * f32(scale[k])
        cmax = (f32(clip[2 + k]) - f32(display_pos[k])) * f32(scale[k])
        cmin = f32(0) if cmin < 0 else cmin
        cmax = f32(extent) if cmax > extent else cmax
        if not cmax > cmin:
            return None
        lo = int(cmin)
        box.append((lo, lo + int(f32(cmax - cmin))))
    return box[0][0], box[1][0], box[0][1], box[1][1]


def covers(P, p):
    """the point p against the triangle P (three points of Fractions)"""
    area = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0])
    if area == 0:
        return False
    for k in range(3):
        a, b, c = P[k], P[(k + 1) % 3], P[(k + 2) % 3]
        side = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        inner = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])  # the third vertex's side: the inside
        if side * inner < 0:
            return False
        if side == 0:
            if a[1] == b[1]:
                owns = c[1] > a[1]  # a top edge: horizontal, the triangle below (y grows downwards)
            else:
                x_on_edge = a[0] + (b[0] - a[0]) * (c[1] - a[1]) / (b[1] - a[1])
                owns = c[0] > x_on_edge  # a left edge: the triangle to its right
            if not owns:
                return False
    return True


def weights(P, p):
    """the barycentric weights of p (exact, then float64)"""
    def cross(a, b, c):
        return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    area = cross(P[0], P[1], P[2])
    return float(cross(p, P[1], P[2]) / area), float(cross(P[0], p, P[2]) / area), float(cross(P[0], P[1], p) / area)


def sample(texture, u, v):
    """bilinear, clamp to edge, no mips -> (r, g, b, a) in float64"""
    texels, w, h, fmt = texture
    texels = np.asarray(texels, dtype=np.float64) / 255.0
    s, t = u * w - 0.5, v * h - 0.5
    i, j = math.floor(s), math.floor(t)
    a, b = s - i, t - j
    def at(x, y):
        x, y = min(max(x, 0), w - 1), min(max(y, 0), h - 1)
        return np.array([1.0, 1.0, 1.0, texels[y, x]]) if fmt == 1 else texels[y, x]
    top = at(i, j) * (1 - a) + at(i + 1, j) * a
    bot = at(i, j + 1) * (1 - a) + at(i + 1, j + 1) * a
    return top * (1 - b) + bot * b


def channels(word, fmt):
    """a texel word -> float64 (r, g, b, a)"""
    c = [((int(word) >> s) & 255) / 255.0 for s in (0, 8, 16, 24)]
    return np.array([c[2], c[1], c[0], c[3]] if fmt == 0 else c)


def word(rgba, fmt):
    q = [int(round(min(max(float(c), 0.0), 1.0) * 255.0)) for c in rgba]  # round(): ties to even
    if fmt == 0:
        q = [q[2], q[1], q[0], q[3]]
    return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24)


def paint(image, fmt, lst):
    """-> (the image after, fragments per pixel)"""
    out = np.array(image, dtype=np.uint32)
    h, w = out.shape
    layers = np.zeros((h, w), np.uint32)
    dp, sc = lst["display_pos"], lst["scale"]
    for cmd in lst["cmds"]:
        if cmd["elem_count"] == 0:
            continue
        box = clip_box(cmd["clip_rect"], dp, sc, w, h)
        if box is None:
            continue
        texture = lst["textures"][cmd["texture"]]
        for t in range(cmd["elem_count"] // 3):
            vs = [lst["vertices"][int(cmd["vtx_offset"]) + int(lst["indices"][int(cmd["idx_offset"]) + 3 * t + k])] for k in range(3)]
            P = [(snapped(v["pos"][0], dp[0], sc[0]), snapped(v["pos"][1], dp[1], sc[1])) for v in vs]
            if any(c is None for pt in P for c in pt):
                continue
            xs, ys = [pt[0] for pt in P], [pt[1] for pt in P]
            x_lo, x_hi = max(math.floor(min(xs)) - 1, box[0]), min(math.ceil(max(xs)) + 1, box[2])
            y_lo, y_hi = max(math.floor(min(ys)) - 1, box[1]), min(math.ceil(max(ys)) + 1, box[3])
            cols = [channels(v["col"], 1) for v in vs]
            for j in range(y_lo, y_hi):
                for i in range(x_lo, x_hi):
                    p = (Fraction(2 * i + 1, 2), Fraction(2 * j + 1, 2))
                    if not covers(P, p):
                        continue
                    layers[j, i] += 1
                    w0, w1, w2 = weights(P, p)
                    u = w0 * float(vs[0]["uv"][0]) + w1 * float(vs[1]["uv"][0]) + w2 * float(vs[2]["uv"][0])
                    v = w0 * float(vs[0]["uv"][1]) + w1 * float(vs[1]["uv"][1]) + w2 * float(vs[2]["uv"][1])
                    src = (w0 * cols[0] + w1 * cols[1] + w2 * cols[2]) * sample(texture, u, v)
                    dst = channels(out[j, i], fmt)
                    a = src[3]
                    rgba = [src[0] * a + dst[0] * (1 - a), src[1] * a + dst[1] * (1 - a), src[2] * a + dst[2] * (1 - a), a + dst[3] * (1 - a)]
                    out[j, i] = word(rgba, fmt)
    return out, layers
