"""The deferred lighting pass stated a second time: from the scene's geometry, in float64.

Like raster_ref.py it imports nothing of the package and loads no library.  It shares the contract's DEFINITIONS - the
pixel's surface point, the shadow test, the falloff of a point light, the stores - and none of its operation order.  In
particular it never reads a depth plane and never unprojects: C17 reconstructs a position from (pixel centre, depth texel)
through an inverse matrix, the reference takes THE POINT OF THE TRIANGLE the pixel shows, the parent triangle's
perspective-correct world position at the pixel centre,

    exact path (raster_ref.Tri):          P = sum b_i P_i / w_i  /  sum b_i / w_i      b_i the areas' ratios on the snapped vertices
    clipped path (raster_ref.ClippedTri): P = sum mu_i P_i  /  sum mu_i                mu_i the coordinates of the pixel's ray

with P_i = world (p_i, 1) and w_i the last row of viewproj at P_i, both in float64 from the float32 inputs taken as exact
reals.  The normal is world (n, 0), not normalised, interpolated the same way; the albedo is the face's vertex colour
times the colour factor (flat material, white texel).  Which face a pixel shows is raster_ref's coverage and, among the
covering faces, the largest float64 depth (reversed Z).

WHAT THE LIBRARIES ARE HANDED, AND WHAT IT DEVIATES BY.  A library's position is the point at (pixel centre, its depth
texel).  The reference's point P projects - forward, through viewproj, in float64 - to a window position and a depth
of its own.  They differ from (pixel centre, depth texel) by known amounts, none of them a rounding of C17-C19:
  * the window position by the snap to 1/256 px (the b_i are the snapped triangle's) and by the float32 roundings of the
    vertex stage (the clip coordinates the cases hand over are float32): `win`, measured per pixel;
  * the depth by those, `geo` (the vertices' z/w in float64 against those in float32, at the point's weights), and by the
    roundings of the depth chain C3-C5, raster_ref's own allowance of the depth texel, `depth`.
They reach the position through the partial derivatives of the unprojection.  Those, the magnitudes of C17's chain and
the deviation of the float32 inverse from the true one are the only use of the inv_viewproj the library is handed
(`position_allowance`): it bounds, it never produces a value.

ALLOWANCES follow raster_ref's convention: eps = 2^-24, first-order running forward bounds, every rounding on the path
adds eps times the magnitude of what it rounds, inputs go through the absolute partial derivatives, one further
eps |result| stands for the second-order terms.  The derivations stand next to the code; every value comes with its
magnitude sum, and the rounding part of every allowance is held to a stated multiple of eps times it
(tests/test_light_geom_ref.py).

EITHER/OR is offered only where a rule jumps and the input lies within its allowance of the jump: the shadow comparison,
the shadow window position at a texel boundary or the map's edge, q.w at 0 (`Ref.shadow_alt`: both colours are
admissible), and the winner where the two largest depths are closer than the sum of their allowances or a clipped
triangle's band covers the pixel (`Ref.offered`: the pixel is not checked).  The falloff is continuous at d2 = r2 and the
cosine at n.v = 0, so those need no such rule; their first-order terms are kept on both sides of n.v = 0.

WRONG names a deliberately wrong variant of one rule (VARIANTS; tests/test_light_geom_ref.py shows each is caught)."""
import numpy as np

import raster_ref as RR

EPS = RR.EPS
RGBA16F, RGBA8 = 0, 1
SUN_FLOOR = float(np.float32(0.1))  # the contract's 0.1f
WRONG = None
VARIANTS = ("corner_sample", "window_y_up", "inverse_transposed", "linear_falloff", "no_plus_one", "normalised_normal",
            "lights_skip_shadowed", "shadow_texel_round", "shadow_bias_sign", "shadow_outside_is_dark", "shadowed_is_black")
K_POSITION = 9   # rounding part of the position allowance <= 9 eps * its magnitude sum (position_allowance)
K_LIGHT = 36     # one light's term <= 36 eps * its magnitude sum; + 1 per accumulating fma (shade)
K_SUN = 8


def is_wrong(name):
    assert name in VARIANTS
    return WRONG == name


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def matrix(m16, camera=True):
    """column-major float[16] -> the 4 x 4 that multiplies column vectors"""
    a = _f64(m16).reshape(4, 4)
    return a if (camera and is_wrong("inverse_transposed")) else a.T


class Mesh:
    """consecutive vertex triples are triangles; colour = vertex colour * colour factor, constant over the mesh"""

    def __init__(self, positions, normals, color, world, clip):
        self.positions, self.normals, self.color, self.world = _f64(positions), _f64(normals), _f64(color)[:3], world
        self.clip = np.asarray(clip, dtype=np.float32)  # (n, 4): what the vertex stage (C0, C1) computes in float32


class Lighting:
    def __init__(self, inv_viewproj, ambient, sun_dir, sun_color, lights=None, shadow=None, shadow_viewproj=None, bias=0.0, ao=None):
        """lights: a record array with position, radius, color, intensity; shadow: the map as read back (Hs, Ws) float32;
        ao: the ambient plane as read back (H, W) or None"""
        self.inv_viewproj = inv_viewproj
        self.ambient, self.sun_dir, self.sun_color = _f64(ambient), _f64(sun_dir), _f64(sun_color)
        self.lights, self.shadow, self.shadow_viewproj, self.bias, self.ao = lights, shadow, shadow_viewproj, float(np.float32(bias)), ao


# ---------------------------------------------------------------- which face, and where on it
def _weights(t, fx, fy):
    """screen-space weights of the three vertices (in the caller's vertex order) at window position (fx, fy), in pixels;
    for a clipped triangle mu_i w_i, the same thing up to their sum"""
    if isinstance(t, RR.Tri):
        X, Y = t.X.astype(np.float64), t.Y.astype(np.float64)  # |coordinates| < 2^17: every product below is exact
        PX, PY = fx * 256.0, fy * 256.0
        cr = lambda ax, ay, bx, by, cx, cy: (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
        T = cr(X[0], Y[0], X[1], Y[1], X[2], Y[2])
        b1, b2 = cr(X[0], Y[0], PX, PY, X[2], Y[2]) / T, cr(X[0], Y[0], X[1], Y[1], PX, PY) / T
        s = [1.0 - b1 - b2, b1, b2]
        return [s[0], s[2], s[1]] if t.area2 < 0 else s  # Tri relabels vertices 1, 2 of a negative area
    return [t._eval(t.N[i], fx - 0.5, fy - 0.5) * t.c[i, 3] for i in range(3)]


class Face:
    def __init__(self, mesh, k, viewproj, width, height):
        i = slice(3 * k, 3 * k + 3)
        W = matrix(mesh.world, camera=False)
        self.P = np.concatenate([mesh.positions[i], np.ones((3, 1))], axis=1) @ W.T          # world (p, 1)
        self.n = mesh.normals[i] @ W[:3, :3].T                                                 # world (n, 0)
        self.n_in = 3 * EPS * (np.abs(mesh.normals[i]) @ np.abs(W[:3, :3]).T).max(axis=0)     # C1's three-term chain, per component
        self.color, self.clip = mesh.color, mesh.clip[i]
        self.c64 = self.P @ viewproj.T                                                         # the true clip coordinates
        if not is_wrong("inverse_transposed"):
            # the hand-over: the float32 clip coordinates are the vertex stage's of these inputs (mvp = viewproj x world, then
            # mvp (p, 1): two four-term chains, 8 roundings of magnitudes bounded by |viewproj| |world| |(p, 1)|)
            mag = np.abs(np.concatenate([mesh.positions[i], np.ones((3, 1))], axis=1)) @ np.abs(W).T @ np.abs(viewproj).T
            assert np.all(np.abs(self.clip.astype(np.float64) - self.c64) <= 10 * EPS * mag), "clip coordinates are not viewproj world p"
            self.d_clip = 10 * EPS * mag  # (3, 4): what a float32 clip coordinate may differ from the true one by
        kind = RR.ClippedTri if RR.routed_to_clipper(self.clip, width, height) else RR.Tri
        # the normal and the colour travel as raster_ref's u, v do (C6): three triangles with them in place of uv
        attrs = [(self.n[:, 0], self.n[:, 1]), (self.n[:, 2], self.color[0] + 0 * self.n[:, 2]), (self.color[1] + 0 * self.n[:, 2], self.color[2] + 0 * self.n[:, 2])]
        self.tris = [kind(self.clip, np.stack(a, axis=1).astype(np.float32), width, height) for a in attrs]
        self.t = self.tris[0]
        self.clipped = kind is RR.ClippedTri
        self.empty = self.clipped and self.t.empty

    def surface(self, px, py, height):
        """world position and normal at the centres of pixels (px, py), by the perspective-correct weights; the deviation of
        the point's depth (module docstring, `geo`); the window position the point is meant to lie at"""
        fx, fy = px + 0.5, py + 0.5
        if is_wrong("corner_sample"):
            fx, fy = fx - 0.5, fy - 0.5
        if is_wrong("window_y_up"):
            fy = height - fy
        s = _weights(self.t, fx, fy)
        w = self.c64[:, 3]
        lam = np.stack([s[i] / w[i] if w[i] != 0.0 else 0.0 * s[i] for i in range(3)], axis=1)
        lam = lam / lam.sum(axis=1, keepdims=True)
        # what the point's forward depth differs from raster_ref's depth at the same weights by: both are screen-linear in
        # z_i / w_i, the point's of the true clip coordinates, raster_ref's of the float32 ones
        sn = np.stack(s, axis=1) / sum(s)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            dzs = np.where(w != 0.0, self.c64[:, 2] / w, 0.0) - np.where(self.clip[:, 3] != 0, self.clip[:, 2].astype(np.float64) / self.clip[:, 3].astype(np.float64), 0.0)
        return lam @ self.P[:, :3], lam @ self.n, np.abs(sn @ dzs), fx, fy, self._window_bound(sn, fx, fy)

    def _window_bound(self, sn, fx, fy):
        """A PRIORI, in NDC per axis: how far the point's own forward projection may lie from the window position it is meant
        for.  `render` measures that offset (`win`) and holds the measurement to this bound, so that an error in the weights
        cannot hide in its own allowance.
          exact path: the point lies at sum s_i (true window position of vertex i), the pixel centre at sum s_i (snapped
            position): each snapped vertex is at most 1/512 px off the float32 one per axis (+ the fma of C3, 4 eps of the
            extent), and that at most (d_x + |ndc| d_w) / w off the true one, d the vertex stage's 10 eps bound.
          clipped path: no snap enters mu_i; p^ = sum mu_i v_i holds for the float32 v_i, the true ones move it by sum mu_i
            dv_i, and the division by its third component gives sum |mu_i| (d_x,i + |ndc| d_w,i) to first order."""
        if not hasattr(self, "d_clip"):
            return None
        w32, d = np.abs(self.clip[:, 3].astype(np.float64)), self.d_clip
        ndc_p = np.stack([fx * 2.0 / self.t.width - 1.0, fy * 2.0 / self.t.height - 1.0], axis=1)
        out = np.zeros_like(ndc_p)
        for a, extent in ((0, self.t.width), (1, self.t.height)):
            if self.clipped:
                mu = np.abs(sn) / np.where(w32 > 0, w32, np.inf)[None, :]
                out[:, a] = (mu * (d[None, :, a] + np.abs(ndc_p[:, a:a + 1]) * d[None, :, 3])).sum(axis=1) * (1 + 1e-6) + 16 * EPS
            else:
                ndc_v = np.abs(self.clip[:, a].astype(np.float64)) / w32
                per = (1.0 / 512.0 + 4 * EPS * extent) * 2.0 / extent + (d[:, a] + ndc_v * d[:, 3]) / w32
                out[:, a] = np.abs(sn) @ per
        return out

    def plane_allowance(self, px, py):
        """what the NORMAL and ALBEDO texels of a float32 G-buffer may differ from the exact ones by: raster_ref's allowance of
        a perspective-correct attribute (C6; on the clipped path with its cut-vertex and snap terms), + the vertex value's
        own roundings (C1: n' three, colour one), which an interpolation with weights that sum to 1 passes on at most once"""
        a = [t.attributes(px, py) for t in self.tris]
        dn = np.stack([a[0]["u"][1], a[0]["v"][1], a[1]["u"][1]], axis=1) + self.n_in[None, :]
        dc = np.stack([a[1]["v"][1], a[2]["u"][1], a[2]["v"][1]], axis=1) + EPS * self.color[None, :]
        return dn, dc


# ---------------------------------------------------------------- allowance of the position
def position_allowance(inv_viewproj, viewproj, width, height, px, py, P, depth, d_depth, d_geo, d_win):
    """What C17's float32 position may differ from the surface point P by -> {"round", "depth", "geo", "win", "inverse"} (n, 3)
    each, and the magnitude sum (n, 3).  THE ONLY USE OF THE INVERSE MATRIX: magnitudes and partial derivatives.

    C17: v = (xn, yn, z, 1), h_r = fma chain of inv[r][c] v_c, p_r = h_r * (1 / h_w).
      xn = fma(px + 1/2, kx, -1), kx = fl(2/W): the quotient's and the fma's rounding      dxn = eps ((px + 1/2) kx + |xn|)
      h_r: four roundings, each of a partial sum <= S_r = sum_c |inv[r][c]| m_c with m = ((px + 1/2) kx + 1, likewise, z, 1)
           (the magnitude sum: it bounds the cancellation, in h_w most of all)              dh_r = 4 eps S_r + sum_c |inv[r][c]| dv_c
           and |inv[r][0]| dxn <= 2 eps |inv[r][0]| m_0, likewise yn: together            <= 6 eps S_r
      p_r = h_r * fl(1/h_w): the reciprocal's and the product's rounding, + 1               dp_r = (dh_r + |p_r| dh_w) / |h_w| + 3 eps |p_r|
      magnitude sum M_r = (S_r + |p_r| S_w) / |h_w| >= |p_r|, so the rounding part is <= 9 eps M_r.
    Inputs, through the same partials |inv[r][c]| / |h_w| and |p_r| |inv[3][c]| / |h_w|:
      depth: the depth texel's allowance (raster_ref: the chain C3-C5; on the clipped path its cut-vertex and snap terms).
             Under the reversed projection (z_near = 10000, z_far = 0.1) h_w is affine in z and shrinks with the distance,
             so this grows with distance^2: per pixel, not bounded once.
      geo, win: the known deviations of P's own forward depth and window position (module docstring); the measured window
             offset is held to its a-priori bound (`Face._window_bound`: 1/512 px of snap + the vertex stage's roundings).
      inverse: the float32 inverse is not the inverse.  E = inv viewproj - I in float64; the true inverse is (I + E)^-1 inv, so
             the true h is h - E h to first order: dh_r = sum_c |E[r][c]| |h_c|."""
    inv, vp = matrix(inv_viewproj), viewproj
    prod = inv @ vp  # (the pass divides by h.w: a multiple of the inverse serves, and is measured as one)
    E = np.abs(prod / prod[3, 3] - np.eye(4))
    kx, ky = float(np.float32(2.0) / np.float32(width)), float(np.float32(2.0) / np.float32(height))
    xn, yn = (px + 0.5) * kx - 1.0, (py + 0.5) * ky - 1.0
    one = np.ones_like(xn)
    v = np.stack([xn, yn, depth, one], axis=1)
    m = np.stack([(px + 0.5) * kx + 1.0, (py + 0.5) * ky + 1.0, np.abs(depth), one], axis=1)
    h = v @ inv.T
    S = m @ np.abs(inv).T
    hw = np.abs(h[:, 3:4])
    p = np.abs(P)

    def through(dh):
        return (dh[:, :3] + p * dh[:, 3:4]) / hw

    dxy = np.stack([EPS * ((px + 0.5) * kx + np.abs(xn)), EPS * ((py + 0.5) * ky + np.abs(yn))], axis=1)
    out = {"round": through(4 * EPS * S + dxy @ np.abs(inv[:, :2]).T) + 3 * EPS * p}
    for name, dz in (("depth", d_depth), ("geo", d_geo)):
        out[name] = through(dz[:, None] * np.abs(inv[:, 2])[None, :])
    out["win"] = through(np.abs(d_win) @ np.abs(inv[:, :2]).T)
    out["inverse"] = through(np.abs(h) @ E.T)
    return out, through(S)


# ---------------------------------------------------------------- C18, C19
def shadow_test(P, dP, L):
    """-> shadowed (n,) bool, near-a-jump (n,) bool.
    q = shadow_viewproj (P, 1); window (ndc + 1) size / 2; the texel whose unit square holds it; shadowed iff q.w > 0, the
    texel is inside the map and z_ndc + bias < texel.
    Allowance (C18: the C0 chain, 1/q.w, the fma to the window, the product, the sum with the bias):
      dq_r = sum_c |S[r][c]| dP_c + 4 eps sum_c |S[r][c] (P, 1)_c|
      dsx  = (Ws/2) (dq_x + |q_x/q_w| dq_w) / |q_w| + 3 eps (Ws/2) (|q_x/q_w| + 1)
      dsz  = (dq_z + |sz| dq_w) / |q_w| + 3 eps |sz| + eps |sz + bias|"""
    n = len(P)
    if L.shadow is None:
        return np.zeros(n, bool), np.zeros(n, bool)
    S = matrix(L.shadow_viewproj)
    hs, ws = L.shadow.shape
    P1 = np.concatenate([P, np.ones((n, 1))], axis=1)
    q = P1 @ S.T
    dq = dP @ np.abs(S[:, :3]).T + 4 * EPS * (np.abs(P1) @ np.abs(S).T)
    front = q[:, 3] > 0.0
    qw = np.where(front, q[:, 3], 1.0)
    near = np.abs(q[:, 3]) <= dq[:, 3]
    win, dwin = [], []
    for k, size in ((0, ws), (1, hs)):
        ndc = q[:, k] / qw
        win.append((ndc + 1.0) * size / 2.0)
        dwin.append(size / 2.0 * (dq[:, k] + np.abs(ndc) * dq[:, 3]) / qw + 3 * EPS * size / 2.0 * (np.abs(ndc) + 1.0))
    sz = q[:, 2] / qw
    dsz = (dq[:, 2] + np.abs(sz) * dq[:, 3]) / qw + 3 * EPS * np.abs(sz) + EPS * np.abs(sz + L.bias)
    z = sz - L.bias if is_wrong("shadow_bias_sign") else sz + L.bias
    plane = L.shadow.astype(np.float64)

    def outcome(wx, wy, zz):
        if is_wrong("shadow_texel_round"):
            wx, wy = wx + 0.5, wy + 0.5
        tx, ty = np.floor(wx), np.floor(wy)
        inside = (tx >= 0) & (tx < ws) & (ty >= 0) & (ty < hs)
        texel = plane[np.clip(ty, 0, hs - 1).astype(np.int64), np.clip(tx, 0, ws - 1).astype(np.int64)]
        dark = front & inside & (zz < texel)
        return dark | (front & ~inside) if is_wrong("shadow_outside_is_dark") else dark

    shadowed = outcome(win[0], win[1], z)
    # a jump within reach: some window position within (dsx, dsy) of the point's and some depth within dsz of its own give
    # the other answer.  The texel squares the box of allowances touches are those of its corners while dsx, dsy < 1/2; a
    # point so close to the light's plane that they are not is offered outright, unless its whole box lies off the map.
    on_map = (win[0] + dwin[0] >= 0) & (win[0] - dwin[0] < ws) & (win[1] + dwin[1] >= 0) & (win[1] - dwin[1] < hs)
    near |= front & on_map & ((dwin[0] >= 0.5) | (dwin[1] >= 0.5))
    for ox in (-1.0, 1.0):
        for oy in (-1.0, 1.0):
            for oz in (-1.0, 1.0):
                near |= outcome(win[0] + ox * dwin[0], win[1] + oy * dwin[1], z + oz * dsz) != shadowed
    return shadowed, near


def shade(P, dP, n, dn, c, dc, shadowed, ao, L):
    """-> rgb (n, 3), {"in": what the inputs' allowances carry, "round": C18/C19's own roundings} (n, 3) each, the magnitude
    sum (n, 3), and the number of lights whose term is not zero (n,).

    SUN (C18).  d = n . L: three roundings                           dd = sum |L_k| dn_k + 3 eps sum |n_k L_k|
      light = max(d, 0.1), or 0.1 when shadowed (1-Lipschitz)        dl = dd where d + dd > 0.1 and not shadowed
      a0 = fma(c light, sw, (c amb) [ao]): the products and the fma  da0 = dc (light |sw| + amb ao) + c |sw| dl + eps (c light |sw| + 2 c amb ao + |a0|)
      magnitude sum c |sw| max(light, sum |n_k L_k|) + c amb ao (the sum where d counts: it carries the cancellation in n . L);
      the rounding part is <= 3 + 4 = 7 eps of it, and the closing eps |rgb| makes K_SUN = 8.
    POINT LIGHT (C19), with v = pl - P, for d2 < r2:
      v_k: one rounding                                              dv = dP + eps |v|
      d2 = sum v_k^2: three roundings of positive partial sums       dd2 = 2 sum |v_k| dv_k + 3 eps d2                    (5 eps d2)
      ndl = n . v                                                    dndl = sum (|n_k| dv_k + |v_k| dn_k) + 3 eps sum |n_k v_k|   (4 eps N, N = sum |n_k v_k|)
      u = d2 / fl(radius^2): r2's rounding and the quotient's        du = dd2 / r2 + 2 eps u                              (7 eps u)
      t = 1 - u                                                      dt = du + eps |t|                                    (8 eps (1 + u))
      tt = t t                                                       dtt = 2 |t| dt + eps tt                              (17 eps |t| (1 + u))
      s = sqrt(d2)                                                   ds = dd2 / (2 s) + eps s                             (3.5 eps s)
      g = ndl / s                                                    dg = dndl / s + |g| ds / s + eps |g|                 (8.5 eps N / s)
      e = d2 + 1                                                     de = dd2 + eps e                                     (6 eps e)
      f = tt / e                                                     df = dtt / e + f de / e + eps f                      (24 eps |t| (1 + u) / e)
      k = (g f) intensity: two roundings                             dk = intensity (f dg + g df + eps g f) + eps k       (34.5 eps)
      a = (c color) k: the product's rounding                        da = color k dc + c color dk + eps a                 (35.5 eps)
      magnitude sum of a: c color intensity (N / s) (|t| (1 + u) / e); K_LIGHT = 36.  It carries the cancellations in n . v
      and in 1 - u, which is why no rule is needed at n . v = 0 or d2 = r2: dg is kept where ndl <= 0 (there g = 0).
    Each accumulating fma rounds a partial sum of non-negative terms: eps times the running sum, per light with a term.
    One further eps |rgb| for the second order."""
    N = len(P)
    if is_wrong("normalised_normal"):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    sw, sun = abs(L.sun_color[3]), L.sun_dir[:3]
    d = n @ sun
    dark = 0.0 if is_wrong("shadowed_is_black") else SUN_FLOOR
    light = np.where(shadowed, dark, np.maximum(d, SUN_FLOOR))[:, None]
    amb = L.ambient[None, :3] * (ao[:, None] if ao is not None else 1.0)
    rgb = c * light * L.sun_color[3] + c * amb
    lit = ~shadowed & (d + dn @ np.abs(sun) + 3 * EPS * (np.abs(n) @ np.abs(sun)) > SUN_FLOOR)
    mag, count = c * sw * np.where(lit, np.maximum(light[:, 0], np.abs(n) @ np.abs(sun)), light[:, 0])[:, None] + c * amb, np.zeros(N, np.int64)
    sun_rgb, pl = rgb, None
    lights = L.lights
    if lights is not None and len(lights):
        lp, lr = _f64(lights["position"]), _f64(lights["radius"])
        r2 = lr * lr
        keep = np.nonzero((((lp[None, :, :] - P[:, None, :]) ** 2).sum(-1) < r2[None, :]).any(axis=0))[0]
        lp, r2, lc, li = lp[keep], r2[keep][None, :], _f64(lights["color"])[keep], _f64(lights["intensity"])[keep][None, :]
        v = lp[None, :, :] - P[:, None, :]
        d2 = (v * v).sum(-1)
        reach = d2 < r2
        ndl, nv = (n[:, None, :] * v).sum(-1), (np.abs(n)[:, None, :] * np.abs(v)).sum(-1)
        u = d2 / r2
        t = 1.0 - (np.sqrt(u) if is_wrong("linear_falloff") else u)
        s = np.sqrt(d2)
        g = np.maximum(ndl, 0.0) / s
        e = d2 if is_wrong("no_plus_one") else d2 + 1.0
        f = t * t / e
        k = np.where(reach, g * f * li, 0.0)
        if is_wrong("lights_skip_shadowed"):
            k = np.where(shadowed[:, None], 0.0, k)
        cc = c[:, None, :] * lc[None, :, :]
        a = cc * k[:, :, None]
        rgb = rgb + a.sum(axis=1)
        running = mag[:, None, :] + np.cumsum(a, axis=1)
        mag = mag + (cc * np.where(reach, li * (nv / s) * (np.abs(t) * (1.0 + u) / e), 0.0)[:, :, None]).sum(axis=1)
        count = (k > 0).sum(axis=1)
        pl = True

    def bound(dP, dn, dc, eps):
        """the first-order bound above; it is linear in (dP, dn, dc, eps), so the inputs' share and the roundings' add up"""
        dd = dn @ np.abs(sun) + 3 * eps * (np.abs(n) @ np.abs(sun))
        out = dc * (light * sw + amb) + c * sw * np.where(lit, dd, 0.0)[:, None] + eps * (c * light * sw + 2 * c * amb + np.abs(sun_rgb))
        if pl is None:
            return out + eps * np.abs(rgb)
        dv = dP[:, None, :] + eps * np.abs(v)
        dd2 = 2 * (np.abs(v) * dv).sum(-1) + 3 * eps * d2
        dndl = (np.abs(n)[:, None, :] * dv + np.abs(v) * dn[:, None, :]).sum(-1) + 3 * eps * nv
        dt = dd2 / r2 + 2 * eps * u + eps * np.abs(t)
        dtt = 2 * np.abs(t) * dt + eps * t * t
        ds = dd2 / (2 * s) + eps * s
        dg = np.where(facing, dndl / s + g * ds / s + eps * g, 0.0)
        df = dtt / e + f * (dd2 + eps * e) / e + eps * f
        dk = np.where(reach, li * (f * dg + g * df + eps * g * f) + eps * k, 0.0)
        per = lc[None, :, :] * k[:, :, None] * dc[:, None, :] + cc * dk[:, :, None] + eps * a + eps * running * (k > 0)[:, :, None]
        return out + per.sum(axis=1) + eps * np.abs(rgb)

    if pl:  # n . v within its whole allowance of 0: the cosine's first-order term is kept on both sides
        dv = dP[:, None, :] + EPS * np.abs(v)
        facing = ndl + (np.abs(n)[:, None, :] * dv + np.abs(v) * dn[:, None, :]).sum(-1) + 3 * EPS * nv > 0.0
    zero = np.zeros_like(dP)
    return rgb, {"in": bound(dP, dn, dc, 0.0), "round": bound(zero, zero, zero, EPS)}, mag, count


# ---------------------------------------------------------------- C20
def store_allowance(value, fmt):
    """half an fp16 ulp of the stored value (of the binade |value| lies in; subnormal below 2^-14), or half a unorm8 step
    (+ the rounding of the product with 255)"""
    if fmt == RGBA8:
        return np.full_like(value, 0.5 / 255.0 + 2 * EPS)
    return 0.5 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(value), 2.0 ** -14))) - 10)


def stored(value, fmt):
    """the reference's colour as the target shows it: fp16 is compared as it is, unorm8 after the clamp"""
    return np.clip(value, 0.0, 1.0) if fmt == RGBA8 else value


def decode(texels, fmt):
    """a colour target as read back (fp16 bit patterns or unorm8) -> float64 (H, W, 4)"""
    texels = np.asarray(texels)
    return texels.astype(np.float64) / 255.0 if fmt == RGBA8 else texels.view(np.float16).astype(np.float64)


# ---------------------------------------------------------------- a whole pass
class Ref:
    """Over the winner pixels (ys, xs in row-major order): face, P, normal, albedo, depth; tolP[name] and magP for the
    position; rgb, tol (the whole allowance, the store's half step included), tol_parts, mag, lights; shadowed, shadow_alt
    and rgb_alt / tol_alt for the pixels whose shadow test is offered either way.  Over the target: covered (some face
    covers the pixel, or a band offers it), offered (the winner is not decided: not checked), winner."""


def render(width, height, viewproj16, meshes, lighting, fmt=RGBA16F):
    vp = matrix(viewproj16)
    faces = [Face(m, k, vp, width, height) for m in meshes for k in range(len(m.positions) // 3)]
    faces = [f for f in faces if not f.empty]
    z_all = np.full((len(faces), height, width), -np.inf)
    dz_all = np.zeros((len(faces), height, width))
    offered = np.zeros((height, width), bool)
    for k, f in enumerate(faces):
        cov = f.t.coverage()
        if f.clipped:
            band = f.t.offered()
            offered |= band
            cov &= ~band
        ys, xs = np.nonzero(cov)
        if len(ys):
            z_all[k, ys, xs], dz_all[k, ys, xs], _ = f.t.attributes(xs, ys)["depth"]
    owner = np.where(np.isfinite(z_all.max(axis=0)), z_all.argmax(axis=0), -1) if faces else np.full((height, width), -1)
    top = np.take_along_axis(z_all - dz_all, np.maximum(owner, 0)[None], axis=0)[0]   # the winner's lower end
    rivals = ((z_all + dz_all >= top[None]) & np.isfinite(z_all)).sum(axis=0)          # the faces whose upper end reaches it
    ref = Ref()
    ref.covered = (owner >= 0) | offered
    ref.offered = offered | ((owner >= 0) & (rivals > 1))
    ref.winner = (owner >= 0) & ~ref.offered
    ref.ys, ref.xs = np.nonzero(ref.winner)
    n = len(ref.ys)
    ref.face = owner[ref.ys, ref.xs]
    ref.P, ref.normal, ref.albedo = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    dn, dc = np.zeros((n, 3)), np.zeros((n, 3))
    ref.depth, d_depth, d_geo, d_win = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, 2))
    for k, f in enumerate(faces):
        m = ref.face == k
        if not m.any():
            continue
        px, py = ref.xs[m], ref.ys[m]
        ref.P[m], ref.normal[m], d_geo[m], fx, fy, bound = f.surface(px, py, height)
        ref.albedo[m] = f.color[None, :]
        dn[m], dc[m] = f.plane_allowance(px, py)
        ref.depth[m], d_depth[m], _ = f.t.attributes(px, py)["depth"]
        # P's own forward projection: where it lies in the window, against where it is meant to lie
        q = np.concatenate([ref.P[m], np.ones((int(m.sum()), 1))], axis=1) @ vp.T
        d_win[m] = np.stack([q[:, 0] / q[:, 3] - (fx * 2.0 / width - 1.0), q[:, 1] / q[:, 3] - (fy * 2.0 / height - 1.0)], axis=1)
        assert bound is None or np.all(np.abs(d_win[m]) <= bound), "the point does not project to where it is meant to lie"
    ref.tol_normal, ref.tol_albedo = dn, dc
    px, py = ref.xs.astype(np.float64), ref.ys.astype(np.float64)
    ref.tolP, ref.magP = position_allowance(lighting.inv_viewproj, vp, width, height, px, py, ref.P, ref.depth, d_depth, d_geo, d_win)
    ref.dP = sum(ref.tolP.values())
    ao = lighting.ao.astype(np.float64)[ref.ys, ref.xs] if lighting.ao is not None else None
    ref.shadowed, ref.shadow_alt = shadow_test(ref.P, ref.dP, lighting)
    half = lambda v, t: store_allowance(np.abs(v) + t, fmt)  # the binade the float32 result may lie in
    ref.rgb, ref.tol_parts, ref.mag, ref.lights = shade(ref.P, ref.dP, ref.normal, dn, ref.albedo, dc, ref.shadowed, ao, lighting)
    ref.tol = ref.tol_parts["in"] + ref.tol_parts["round"]
    ref.tol = ref.tol + half(stored(ref.rgb, fmt), ref.tol)
    ref.rgb_alt, ref.tol_alt = ref.rgb.copy(), ref.tol.copy()
    k = np.nonzero(ref.shadow_alt)[0]
    if len(k):
        rgb, parts, _, _ = shade(ref.P[k], ref.dP[k], ref.normal[k], dn[k], ref.albedo[k], dc[k], ~ref.shadowed[k], ao[k] if ao is not None else None, lighting)
        ref.rgb_alt[k], ref.tol_alt[k] = rgb, parts["in"] + parts["round"] + half(stored(rgb, fmt), parts["in"] + parts["round"])
    ref.fmt = fmt
    return ref
