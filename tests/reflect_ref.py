"""Test-side helpers of the reflection pass (include/svr_reflect.h): build and run tests/native/reflect_ref.cpp, the scalar
restatement of DESIGN C73-C79; analytic scenes ray-cast in fp64 into a G-buffer (a floor, a back wall, a box and sky); and
the fp64 statements of the same pass written from the header's definitions, trace64 (C73-C77) and resolve64 (C78, C79).
Colour targets travel as uint16 [H, W, 4] arrays of fp16 bit patterns, depth as float32 [H, W] (reversed-Z: 1 at the near
plane, bits 0 where nothing was drawn), the normal and albedo planes as float32 [H, W, 4].  Matrices are 4 x 4 numpy arrays
in the mathematical convention (M @ column vector); colmajor() gives the 16 floats the C structs hold."""
import functools
import math

import numpy as np

import fog_ref as FR
import native_ref as N
from fog_ref import colmajor, fog_hash, look_at, perspective, random_hdr  # noqa: F401  (re-exported)
from native_ref import SPECIALS, floats, halves  # noqa: F401  (re-exported)

f32 = np.float32
U = 2.0 ** -24
WRONG_VARIANTS = {1: "normal not normalised", 2: "dither dropped", 3: "first sample at i = 0", 4: "thickness test dropped",
                  5: "too deep ends the march", 6: "refinement returns lo", 7: "rint for floor", 8: "Fresnel exponent 4",
                  9: "edge fade at the source pixel", 10: "resolve without depth test", 11: "composite adds", 12: "scissor exit clamped"}
DEFAULTS = dict(max_distance=8.0, steps=16, refine=4, thickness=0.1, f0=0.04, intensity=1.0, distance_fade=0.5, edge_width=0.0, resolve=0,
                depth_tolerance=0.05, frame_index=0)

ref_exe = functools.partial(N.build, "reflect_ref")


class Camera:
    """eye, the view-projection and its inverse as the 16 float32 values the pass takes, and the depth terms of
    glmath.dof_depth_terms for this projection (depth = near / axial distance: 1 / axial = depth / near + 0)"""

    def __init__(self, w, h, eye=(0.3, 1.6, 2.0), target=(0.0, 0.6, -4.0), fov_y=1.0, near=0.5):
        self.w, self.h, self.near = w, h, near
        self.eye = np.asarray(eye, f32)
        self.M = perspective(fov_y, w / h, near) @ look_at(self.eye.astype(np.float64), target)
        self.viewproj = colmajor(self.M)
        self.inv = colmajor(np.linalg.inv(self.M))
        self.inv_z_scale, self.inv_z_bias = f32(1.0 / near), f32(0.0)

    def args(self):
        """what run_ref, trace64 and Renderer.reflect_pass take first"""
        return self.viewproj, self.inv, self.eye, self.inv_z_scale, self.inv_z_bias


# ---------------------------------------------------------------- analytic scenes, ray-cast in fp64
STRIPES = np.array([[4.0, 0.25, 0.25], [0.25, 4.0, 0.25], [0.25, 0.25, 4.0], [3.0, 3.0, 0.25], [0.25, 3.0, 3.0], [3.0, 0.25, 3.0]])
STRIPE_W = 1.5  # world units
FLOOR_RGB, BOX_RGB, SKY_RGB = (0.5, 0.5, 0.5), (2.0, 1.0, 0.5), (0.25, 0.5, 1.0)


def stripe_of(x):
    """the index of the wall's stripe at world x"""
    return np.floor(np.asarray(x, np.float64) / STRIPE_W).astype(int) % len(STRIPES)


def cast(cam, wall_z=-6.0, wall_h=5.0, box=((-1.6, 0.0, -4.2), (-0.6, 1.2, -3.0)), normal_scale=1.0, seed=None):
    """The G-buffer of a floor (y = 0, z > wall_z), a back wall (z = wall_z, 0 <= y <= wall_h, colour stripes along x), an
    axis-aligned box (None: no box) and sky, seen through the centre of every pixel, in float64 -> dict(color uint16
    [h, w, 4], depth float32 [h, w], normal float32 [h, w, 4], albedo float32 [h, w, 4], kind int [h, w]: 0 sky, 1 floor,
    2 wall, 3 box, point float64 [h, w, 3]).  normal_scale: the length of the stored normals (C74 normalises them); seed:
    a seeded length per pixel in [0.5, 2] times it"""
    w, h = cam.w, cam.h
    Minv, eye = np.linalg.inv(cam.M), cam.eye.astype(np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    q = np.stack([(x + 0.5) * 2.0 / w - 1.0, (y + 0.5) * 2.0 / h - 1.0, np.ones((h, w)), np.ones((h, w))], -1) @ Minv.T
    d = q[..., :3] / q[..., 3:] - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((h, w), np.inf)
    kind = np.zeros((h, w), int)
    nrm = np.zeros((h, w, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -eye[1] / d[..., 1]  # the floor
        p = eye + t[..., None] * d
        ok = (d[..., 1] < 0) & (t > 0) & (p[..., 2] > wall_z)
        best, kind, nrm = np.where(ok, t, best), np.where(ok, 1, kind), np.where(ok[..., None], (0.0, 1.0, 0.0), nrm)
        t = (wall_z - eye[2]) / d[..., 2]  # the wall
        p = eye + t[..., None] * d
        ok = (d[..., 2] < 0) & (t > 0) & (t < best) & (p[..., 1] >= 0) & (p[..., 1] <= wall_h)
        best, kind, nrm = np.where(ok, t, best), np.where(ok, 2, kind), np.where(ok[..., None], (0.0, 0.0, 1.0), nrm)
        if box is not None:  # slabs
            lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
            t0, t1 = (lo - eye) / d, (hi - eye) / d
            tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
            t_in, t_out = tn.max(-1), tf.min(-1)
            ok = (t_in < t_out) & (t_in > 0) & (t_in < best)
            axis = tn.argmax(-1)
            face = -np.sign(np.take_along_axis(d, axis[..., None], -1))[..., 0]
            n_box = np.zeros((h, w, 3))
            np.put_along_axis(n_box, axis[..., None], face[..., None], -1)
            best, kind, nrm = np.where(ok, t_in, best), np.where(ok, 3, kind), np.where(ok[..., None], n_box, nrm)
    hit = kind > 0
    point = eye + np.where(hit, best, 0.0)[..., None] * d
    axial = (np.concatenate([point, np.ones((h, w, 1))], -1) @ cam.M.T)[..., 3]
    depth = np.where(hit, cam.near / np.where(hit, axial, 1.0), 0.0).astype(f32)
    rgb = np.empty((h, w, 3))
    rgb[...] = SKY_RGB
    rgb[kind == 1] = FLOOR_RGB
    rgb[kind == 2] = STRIPES[stripe_of(point[..., 0])][kind == 2]
    rgb[kind == 3] = BOX_RGB
    color = np.concatenate([halves(rgb), np.full((h, w, 1), 0x3c00, np.uint16)], -1)
    scale = np.full((h, w), float(normal_scale))
    if seed is not None:
        scale = scale * np.random.default_rng(seed).uniform(0.5, 2.0, (h, w))
    normal = np.concatenate([nrm * scale[..., None], np.zeros((h, w, 1))], -1).astype(f32)
    albedo = np.concatenate([np.full((h, w, 3), 0.5), hit[..., None].astype(np.float64)], -1).astype(f32)
    return dict(color=color, depth=depth, normal=normal, albedo=albedo, kind=kind, point=point)


# ---------------------------------------------------------------- the restatement
def run_ref(g, viewproj, inv_viewproj, camera, inv_z_scale, inv_z_bias, scissor=None, variant=0, sanitize=False, **kw):
    """reflect_ref (sanitize: its build under the address and undefined-behaviour sanitizers) over the G-buffer g (a dict with color, depth, normal, albedo) -> dict(color: uint16 [H, W, 4] after the
    pass, trace: float32 [sh, sw, 4], t_hit: float32 [sh, sw], hit: int32 [sh, sw, 2] (x, y in the target; -1: a miss))"""
    p = dict(DEFAULTS, **kw)
    color = np.ascontiguousarray(g["color"])
    depth = np.ascontiguousarray(g["depth"], dtype=f32)
    normal, albedo = (np.ascontiguousarray(g[k], dtype=f32) for k in ("normal", "albedo"))
    assert color.dtype == np.uint16 and color.ndim == 3 and color.shape[2] == 4 and depth.shape == color.shape[:2]
    assert normal.shape == color.shape and albedo.shape == color.shape
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, p["steps"], p["refine"], p["resolve"], p["frame_index"] & 0xffffffff, variant, 0], np.uint32)
    par = np.concatenate([np.asarray(viewproj, f32).reshape(16), np.asarray(inv_viewproj, f32).reshape(16), np.asarray(camera, f32).reshape(3),
                          [inv_z_scale, inv_z_bias, p["max_distance"], p["thickness"], p["f0"], p["intensity"], p["distance_fade"], p["edge_width"],
                           p["depth_tolerance"]]]).astype(f32)
    assert par.size == 44
    raw = N.run(ref_exe(sanitize=sanitize), hdr.tobytes() + par.tobytes() + color.tobytes() + depth.tobytes() + normal.tobytes() + albedo.tobytes())
    n, sn = w * h * 8, sw * sh
    assert len(raw) == n + sn * (16 + 4 + 8)
    return dict(color=np.frombuffer(raw[:n], np.uint16).reshape(h, w, 4).copy(),
                trace=np.frombuffer(raw[n:n + sn * 16], f32).reshape(sh, sw, 4).copy(),
                t_hit=np.frombuffer(raw[n + sn * 16:n + sn * 20], f32).reshape(sh, sw).copy(),
                hit=np.frombuffer(raw[n + sn * 20:], np.int32).reshape(sh, sw, 2).copy())


# ---------------------------------------------------------------- the fp64 statements, from the definitions
def san64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, 65504.0), 0.0)


def trace64(g, viewproj, inv_viewproj, camera, inv_z_scale, inv_z_bias, scissor=None, **kw):
    """C73-C77 in float64, written from include/svr_reflect.h's definitions: no fma, no reciprocal, divisions where the
    definitions divide.  Returns dict(trace [sh, sw, 4], t_hit [sh, sw], hit int [sh, sw, 2] (-1: a miss), traced bool
    [sh, sw] (C73), and per ray the quantities the error bounds and the margins of a comparison need: v_len [sh, sw] (|p -
    camera|), d [sh, sw] (n^ . v^) and e_d, its error bound (Margins.ray), and near [sh, sw], the smallest over the ray's evaluated samples, refinement included, of (distance to a
    decision) / (that decision's unit error at the sample), see Margins; near_by [sh, sw, 3] has it by decision: hw = 0, a pixel edge, q; behind_camera [sh, sw]:
    the ray ended at a sample with hw <= 0)."""
    p = dict(DEFAULTS, **kw)
    depth = np.asarray(g["depth"], f32).astype(np.float64)
    normal, albedo = np.asarray(g["normal"], f32), np.asarray(g["albedo"], f32)
    rgb = san64(floats(g["color"])[..., :3])
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    M = np.asarray(viewproj, f32).astype(np.float64).reshape(4, 4).T
    Minv = np.asarray(inv_viewproj, f32).astype(np.float64).reshape(4, 4).T
    cam = np.asarray(camera, f32).astype(np.float64)
    zs, zb = float(f32(inv_z_scale)), float(f32(inv_z_bias))
    maxd, steps, refine = float(f32(p["max_distance"])), int(p["steps"]), int(p["refine"])
    thick, f0, inten, fade, edge = (float(f32(p[k])) for k in ("thickness", "f0", "intensity", "distance_fade", "edge_width"))
    delta = maxd / steps
    frame = p["frame_index"] & 0xffffffff
    mg = Margins(M, cam, w, h)
    out = dict(trace=np.zeros((sh, sw, 4)), t_hit=np.zeros((sh, sw)), hit=np.full((sh, sw, 2), -1), traced=np.zeros((sh, sw), bool),
               v_len=np.zeros((sh, sw)), e_d=np.zeros((sh, sw)), d=np.zeros((sh, sw)), near=np.full((sh, sw), np.inf), near_by=np.full((sh, sw, 3), np.inf), behind_camera=np.zeros((sh, sw), bool), samples=np.zeros((sh, sw), int))
    for y in range(sh):
        for x in range(sw):
            px, py = sx + x, sy + y
            n = normal[py, px, :3].astype(np.float64)
            if albedo[py, px, 3:].view(np.uint32)[0] != 0x3F800000 or np.asarray(g["depth"], f32)[py, px].view(np.uint32) == 0 or not n @ n > 0:
                continue
            out["traced"][y, x] = True
            q = Minv @ np.array([(px + 0.5) * 2.0 / w - 1.0, (py + 0.5) * 2.0 / h - 1.0, depth[py, px], 1.0])
            pos = q[:3] / q[3]
            v = pos - cam
            vv = v @ v
            if not (vv > 0 and math.isfinite(vv)):
                continue
            nh, vh = n / math.sqrt(n @ n), v / math.sqrt(vv)
            d = nh @ vh
            r = vh - 2.0 * d * nh
            h0, dh = M @ np.append(pos, 1.0), M @ np.append(r, 0.0)
            out["v_len"][y, x], out["d"][y, x] = math.sqrt(vv), d
            ray = mg.ray(pos, math.sqrt(vv))
            out["e_d"][y, x] = ray[3]
            near = out["near_by"][y, x]  # by decision: hw = 0, a pixel edge (the scissor's border is one), q = 1 or 1 + thickness

            def sample(t):
                """-> (0 outside / 1 in front / 2 too deep / 3 hit, fx, fy)"""
                out["samples"][y, x] += 1
                hh = h0 + t * dh
                e_h = mg.e_h(ray, t, refine)
                near[0] = min(near[0], abs(hh[3]) / e_h[2])
                if not hh[3] > 0:
                    out["behind_camera"][y, x] = True
                    return 0, -1, -1
                ux, uy = (hh[0] / hh[3] * 0.5 + 0.5) * w, (hh[1] / hh[3] * 0.5 + 0.5) * h
                e_px = mg.e_px(e_h, hh)
                near[1] = min(near[1], abs(ux - round(ux)) / e_px[0], abs(uy - round(uy)) / e_px[1])
                fx, fy = math.floor(ux), math.floor(uy)
                if not (sx <= fx < sx + sw and sy <= fy < sy + sh):
                    return 0, -1, -1
                qq = hh[3] * (depth[fy, fx] * zs + zb)
                e_q = mg.e_q(e_h, hh, qq)
                near[2] = min(near[2], abs(qq - 1.0) / e_q, abs(qq - (1.0 + thick)) / e_q)
                return (3 if qq <= 1.0 + thick else 2) if qq >= 1.0 else 1, fx, fy

            o = (fog_hash(px, py, frame) >> 24) / 256.0
            found = None
            for i in range(1, steps + 1):
                t = (i + o) * delta
                s, fx, fy = sample(t)
                if s == 0:
                    break
                if s == 3:
                    found = (t, fx, fy)
                    break
            out["near"][y, x] = near.min()
            if found is None:
                continue
            t, fx, fy = found
            lo, hi = t - delta, t
            for _ in range(refine):
                mid = 0.5 * (lo + hi)
                s, mx, my = sample(mid)
                if s >= 2:
                    hi, fx, fy = mid, mx, my
                else:
                    lo = mid
            out["near"][y, x] = near.min()
            m = 1.0 - min(max(-d, 0.0), 1.0)
            F = f0 + (1.0 - f0) * m ** 5
            fd = min(max(1.0 - fade * hi / maxd, 0.0), 1.0)
            fe = 1.0
            if edge > 0:
                e = min(fx - sx, sx + sw - 1 - fx, fy - sy, sy + sh - 1 - fy)
                fe = min(max((e + 0.5) / edge, 0.0), 1.0)
            k = min(max(inten * F * fd * fe, 0.0), 1.0)
            out["trace"][y, x] = np.append(k * rgb[fy, fx], k)
            out["t_hit"][y, x] = hi
            out["hit"][y, x] = (fx, fy)
    return out


def resolve64(g, trace, inv_z_scale, inv_z_bias, scissor=None, **kw):
    """C78, C79 in float64 over the given trace texels [sh, sw, 4] -> dict(rgb float64 [sh, sw, 3]: the scissor's colour
    before the store's rounding to a half, near [sh, sw]: the smallest over the pixel's taps of | |iz_j - iz_c| - tol iz_c | over
    the comparison's fp32 error u (|iz_j| + |iz_c| + |iz_j - iz_c| + tol iz_c): the two fma, the difference and the product
    (inf without the resolve); at most 1: the comparison may fall either way in fp32)"""
    p = dict(DEFAULTS, **kw)
    depth = np.asarray(g["depth"], f32).astype(np.float64)
    h, w = depth.shape
    sx, sy, sw, sh = scissor if scissor else (0, 0, w, h)
    iz = (depth * float(f32(inv_z_scale)) + float(f32(inv_z_bias)))[sy:sy + sh, sx:sx + sw]
    I = san64(floats(g["color"])[sy:sy + sh, sx:sx + sw, :3])
    trace = np.asarray(trace, np.float64)
    tol = float(f32(p["depth_tolerance"]))
    near = np.full((sh, sw), np.inf)
    if p["resolve"]:
        acc, ws = np.zeros((sh, sw, 4)), np.zeros((sh, sw))
        ys, xs = np.mgrid[0:sh, 0:sw]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ty, tx = np.clip(ys + dy, 0, sh - 1), np.clip(xs + dx, 0, sw - 1)
                gap = np.abs(iz[ty, tx] - iz)
                counts = (gap <= tol * iz) | ((dy == 0) & (dx == 0))
                if dy or dx:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        err = U * (np.abs(iz[ty, tx]) + np.abs(iz) + gap + tol * np.abs(iz))  # 0: both are 0 exactly, as in fp32
                        near = np.minimum(near, np.where(err > 0, np.abs(gap - tol * iz) / np.where(err > 0, err, 1.0), np.inf))
                acc += np.where(counts[..., None], trace[ty, tx], 0.0)
                ws += counts
    else:
        acc, ws = trace, np.ones((sh, sw))
    kb = acc[..., 3] / ws
    return dict(rgb=san64(acc[..., :3] / ws[..., None] + I * (1.0 - kb[..., None])), near=near)


class Margins:
    """The first-order error bounds of C74-C75 (u = 2^-24), per ray and per sample, as tests/test_reflect_ref.py derives
    them.  M: the view-projection (float64 of the float32 values), cam: the eye, (w, h): the target's extent."""

    def __init__(self, M, cam, w, h):
        self.rows = np.abs(M[[0, 1, 3], :3]).sum(axis=1)       # |row|_1 of the x, y and w rows over a direction or a point
        self.offs = np.abs(M[[0, 1, 3], 3])
        self.cam1 = float(np.abs(cam).sum())
        self.w, self.h = w, h

    def ray(self, pos, v_len):
        """(e_h0 [3], e_dh [3], |h|'s bound [3], e_d) of the ray from pos, v_len = |pos - camera|"""
        p1 = float(np.abs(pos).sum())
        e_p = 8 * U * (p1 + self.cam1 + v_len)                  # a component of p (C17: a 4-term chain, 1 / w, a product)
        e_vh = e_p / v_len + 4 * U                             # a component of v^: the difference, the squares' chain, root, 1 / x, product
        e_d = 1.8 * (3 * U + e_vh) + 3 * U                     # d: |n^|_1, |v^|_1 <= sqrt 3; n^'s components carry 3 u
        e_r = 2 * e_d + 6 * U + e_vh + 2 * U                   # a component of r = fma(-2 d, n^, v^)
        mag = self.rows * p1 + self.offs                       # the largest the chain's partial sums of h0 can be
        return self.rows * e_p + 4 * U * mag, self.rows * e_r + 4 * U * self.rows * 1.8, mag, e_d

    def e_h(self, ray, t, refine):
        """a component (x, y, w) of h = fma(dh, t, h0) at t, with t's own (3 + refine) u"""
        e_h0, e_dh, mag, _ = ray
        return e_h0 + t * e_dh + (3 + refine) * U * t * self.rows * 1.8 + U * (mag + t * self.rows * 1.8)

    def e_px(self, e_h, hh):
        """(x, y): the sample's position in pixels"""
        rw = 1.0 / abs(hh[3])
        ex = (e_h[0] + abs(hh[0]) * rw * e_h[2]) * rw + 3 * U * abs(hh[0]) * rw
        ey = (e_h[1] + abs(hh[1]) * rw * e_h[2]) * rw + 3 * U * abs(hh[1]) * rw
        return 0.5 * self.w * ex + U * self.w, 0.5 * self.h * ey + U * self.h

    def e_q(self, e_h, hh, q):
        """q = hw fma(depth, inv_z_scale, inv_z_bias): hw's error and two roundings"""
        return abs(q) * (e_h[2] / abs(hh[3]) + 3 * U) + 1e-300
