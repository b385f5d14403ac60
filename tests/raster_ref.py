"""A second, independent statement of the fixed-function rules, in numpy and exact integers.

Written from the DEFINITIONS the Vulkan specification gives (as DESIGN.md / SURVEY.md quote them), not from the operation
order of the arithmetic contract DESIGN.md §3: coverage by exact point-in-triangle tests with the top-left rule in its
own words, barycentrics as ratios of areas, perspective-correct attributes as sum(b_i a_i / w_i) / sum(b_i / w_i),
derivatives as differences inside the 2x2 quad, lambda = log2(rho) with the true logarithm, texel filtering on
unnormalised coordinates with REPEAT as "i mod size".  It imports nothing of the package and loads no library.

Beside every value it returns an ALLOWANCE: what an fp32 implementation of the contract's chains C3-C9 may differ by.
eps = 2^-24.  Every allowance is a first-order running forward error bound: each rounding on the path adds eps times the
magnitude of what it rounds, input errors are carried through by the absolute value of the partial derivatives, and one
further eps * |result| stands for the second-order terms ("roundings on the path + 1").  Every chain also returns its
MAGNITUDE SUM, and no allowance exceeds 16 eps times it (asserted by tests/test_raster_ref.py).  The derivations stand
next to the code.  Where a rule is discontinuous (NEAREST texel choice, mip NEAREST level, the mag/min switch) and the
input lies within its allowance of the jump, the reference returns every admissible result (`Ref.alts`).

WRONG names a deliberately wrong variant of one rule (tests/test_raster_ref.py shows that each is caught); None is the
reference.

THE CLIP VOLUME (C2) is stated from its definition too, by `ClippedTri`: a pixel centre is covered iff the ray through
it meets the triangle at a point with w > 0 and 0 <= z <= w there, and the values at it are the parent triangle's
perspective-correct ones.  Nothing of Sutherland-Hodgman, of the order of the planes or of a fan is restated; the only
thing taken from C2's wording is WHICH triangles go through the clipper (`routed_to_clipper`), because the others keep
the exact path above.  The libraries snap the vertices the clipper makes, which the reference cannot know, so a clipped
triangle's coverage carries an either/or band of width tau around its ideal boundary and its values a snap term;
both are derived at `ClippedTri`."""
import math

import numpy as np

EPS = 2.0 ** -24
LOD_POLY = 5e-5  # DESIGN C8: the stated error of the log2 polynomial
NEAREST, LINEAR = 0, 1
WRONG = None
VARIANTS = ("bottom_right", "affine_uv", "taps_floor_u", "floor_lambda", "ceil_extent", "fmod_wrap", "mag_min_swapped",
            "no_near", "no_far", "behind_the_eye", "guard_saturate")
GUARD_PX = 16384.0  # C2: the guard band, in pixels


def is_wrong(name):
    assert name in VARIANTS
    return WRONG == name


# ---------------------------------------------------------------- window coordinates and the snap
def snap(clip, width, height):
    """clip (..., 4) float32 -> (X, Y) int64 in 1/256 pixel, z_s, 1/w in float64, and the distance of x_s*256, y_s*256
    from the nearest rounding tie.  x_s = (x/w + 1) W/2 in float64 (error ~1e-16, nothing beside the fp32 chain's), then
    round to nearest, ties to even."""
    c = np.asarray(clip, dtype=np.float32).astype(np.float64)
    x = (c[..., 0] / c[..., 3] + 1.0) * (width / 2.0) * 256.0
    y = (c[..., 1] / c[..., 3] + 1.0) * (height / 2.0) * 256.0
    if is_wrong("guard_saturate"):
        x, y = np.clip(x, -GUARD_PX * 256.0, GUARD_PX * 256.0), np.clip(y, -GUARD_PX * 256.0, GUARD_PX * 256.0)
    tie = np.minimum(np.abs(x - np.floor(x) - 0.5), np.abs(y - np.floor(y) - 0.5))
    return np.rint(x).astype(np.int64), np.rint(y).astype(np.int64), c[..., 2] / c[..., 3], 1.0 / c[..., 3], tie


def _cross(ax, ay, bx, by, cx, cy):
    """twice the signed area of (a, b, c); exact in int64 (|coordinates| < 2^17 here, products < 2^36)"""
    return (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)


def coverage(X, Y, width, height):
    """Pixels whose centre the triangle covers: (height, width) bool.  Exact integers, either winding, zero area nothing.
    A centre strictly inside is covered.  A centre exactly on an edge is covered iff that edge is a TOP edge - exactly
    horizontal, with the interior below it (window y points down, so the third vertex has the larger y) - or a LEFT edge
    - not horizontal, with the interior to its right (the third vertex lies at larger x than the edge's line at the
    vertex's own y)."""
    X, Y = [int(v) for v in X], [int(v) for v in Y]
    if _cross(X[0], Y[0], X[1], Y[1], X[2], Y[2]) == 0:
        return np.zeros((height, width), bool)
    py, px = np.mgrid[0:height, 0:width].astype(np.int64)
    px, py = px * 256 + 128, py * 256 + 128
    inside = np.ones((height, width), bool)
    for i in range(3):
        a, b, c = (i + 1) % 3, (i + 2) % 3, i
        side_c = _cross(X[a], Y[a], X[b], Y[b], X[c], Y[c])  # which side the interior is on
        side_p = _cross(X[a], Y[a], X[b], Y[b], px, py) * (1 if side_c > 0 else -1)
        horizontal = Y[a] == Y[b]
        top = horizontal and Y[c] > Y[a]
        # x of the edge's line at y = Y[c] is X[a] + (Y[c]-Y[a]) (X[b]-X[a]) / (Y[b]-Y[a]); the comparison without the division
        left = (not horizontal) and ((X[c] - X[a]) * (Y[b] - Y[a]) - (Y[c] - Y[a]) * (X[b] - X[a])) * (1 if Y[b] > Y[a] else -1) > 0
        owns = (top or left) if not is_wrong("bottom_right") else not (top or left)
        inside &= (side_p > 0) | ((side_p == 0) & owns)
    return inside


# ---------------------------------------------------------------- interpolation
def _chain(b1, b2, a, da):
    """Screen-linear interpolation of vertex values a[0..2] (absolute input errors da) at barycentrics b1, b2.
    Value: the definition, b0 a0 + b1 a1 + b2 a2.
    Allowance: the contract evaluates fma(b2, a2-a0, fma(b1, a1-a0, a0)) (C5, C6):
      b_k = float(e_k) * (1 / float(area2)): four roundings, + 1                       db_k  = 5 eps |b_k|
      d_k = a_k - a_0                                                                  dd_k  = da_k + da_0 + eps |d_k|
      inner = b1 d1 + a0, one rounding                                                 di    = |b1| dd1 + |d1| db1 + da0 + eps |inner|
      outer = b2 d2 + inner, one rounding, + 1                                         do    = |b2| dd2 + |d2| db2 + di + 2 eps |outer|
    Magnitude sum: |a0| + |b1| (|a1| + |a0|) + |b2| (|a2| + |a0|).  With da_k <= 2 eps |a_k| this is <= 12 eps of it."""
    d1, d2 = a[1] - a[0], a[2] - a[0]
    val = (1.0 - b1 - b2) * a[0] + b1 * a[1] + b2 * a[2]
    db1, db2 = 5 * EPS * np.abs(b1), 5 * EPS * np.abs(b2)
    inner = a[0] + b1 * d1
    di = np.abs(b1) * (da[1] + da[0] + EPS * abs(d1)) + abs(d1) * db1 + da[0] + EPS * np.abs(inner)
    do = np.abs(b2) * (da[2] + da[0] + EPS * abs(d2)) + abs(d2) * db2 + di + 2 * EPS * np.abs(val)
    mag = abs(a[0]) + np.abs(b1) * (abs(a[1]) + abs(a[0])) + np.abs(b2) * (abs(a[2]) + abs(a[0]))
    return val, do, mag


class Tri:
    """One triangle after the snap.  Vertices 1 and 2 are relabelled when the snapped area is negative: the libraries
    report b1, b2 as the weights of the second and third vertex of the counter-clockwise (positive area2, y down)
    triangle - a naming convention of their output, not a rule; coverage above does not use it."""

    def __init__(self, clip, uv, width, height):
        X, Y, zs, rw, tie = snap(clip, width, height)
        uv = np.asarray(uv, dtype=np.float32).astype(np.float64)
        w = np.asarray(clip, dtype=np.float32).astype(np.float64)[:, 3]
        self.area2 = int(_cross(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
        order = [0, 2, 1] if self.area2 < 0 else [0, 1, 2]
        self.X, self.Y, self.zs, self.rw, self.uv, self.w = X[order], Y[order], zs[order], rw[order], uv[order], w[order]
        self.tie = float(tie.min())
        self.width, self.height = width, height

    def coverage(self):
        return coverage(self.X, self.Y, self.width, self.height)

    def bary(self, px, py):
        """b1, b2 at pixel centres: ratios of areas, exact integers divided once in float64"""
        X, Y = self.X, self.Y
        PX, PY = np.asarray(px, np.int64) * 256 + 128, np.asarray(py, np.int64) * 256 + 128
        T = _cross(X[0], Y[0], X[1], Y[1], X[2], Y[2])
        b1 = _cross(X[0], Y[0], PX, PY, X[2], Y[2]) / float(T)
        b2 = _cross(X[0], Y[0], X[1], Y[1], PX, PY) / float(T)
        return b1, b2

    def attributes(self, px, py):
        """depth, r = 1/w and perspective-correct u, v at pixel centres (extrapolating outside the triangle), each as
        (value, allowance, magnitude sum).
          z_s,i = z_i * (1/w_i): two roundings (C3)              da = 2 eps |z_s,i|;  depth = chain, clamped to [0, 1]
          q_i = 1/w_i: one rounding                              da = eps q_i;        q = chain
          r = 1/q: one rounding, + 1                             dr = dq / q^2 + 2 eps r              magnitude sum magq / q^2
          a'_i = a_i * (1/w_i): two roundings                    da = 2 eps |a'_i|;   a' = chain
          a = a' * r (C6): the product's rounding and r's, + 1   da = da'/q + |a| dq/q + 3 eps |a|    magnitude sum maga'/q + |a| magq/q"""
        b1, b2 = self.bary(px, py)
        out = {"b1": (b1, 5 * EPS * np.abs(b1), np.abs(b1)), "b2": (b2, 5 * EPS * np.abs(b2), np.abs(b2))}
        z, dz, mz = _chain(b1, b2, self.zs, 2 * EPS * np.abs(self.zs))
        out["depth"] = (np.clip(z, 0.0, 1.0), dz, mz)
        q, dq, mq = _chain(b1, b2, self.rw, EPS * np.abs(self.rw))
        out["r"] = (1.0 / q, dq / q ** 2 + 2 * EPS / np.abs(q), mq / q ** 2)
        for k, name in enumerate("uv"):
            a = self.uv[:, k]
            if is_wrong("affine_uv"):
                val, da, ma = _chain(b1, b2, a, 0 * a)
                out[name] = (val, da, ma)
                continue
            ap = a * self.rw
            num, dn, mn = _chain(b1, b2, ap, 2 * EPS * np.abs(ap))
            val = num / q
            out[name] = (val, dn / np.abs(q) + np.abs(val) * dq / np.abs(q) + 3 * EPS * np.abs(val),
                         mn / np.abs(q) + np.abs(val) * mq / np.abs(q))
        return out


# ---------------------------------------------------------------- the clip volume
def routed_to_clipper(clip, width, height):
    """C2's routing, the one thing taken from its wording: a triangle goes through the clipper iff a vertex is beyond
    z = 0 or z = w, or a window coordinate is beyond the guard band.  (A vertex with w <= 0 is beyond z = w or z = 0, or
    has z = w = 0 and no window position: the clipper's too.)"""
    c = np.asarray(clip, dtype=np.float32).astype(np.float64)
    if np.any(c[:, 2] < 0.0) or np.any(c[:, 2] > c[:, 3]) or np.any(c[:, 3] <= 0.0):
        return True
    if is_wrong("guard_saturate"):
        return False
    xs = (c[:, 0] / c[:, 3] + 1.0) * (width / 2.0)
    ys = (c[:, 1] / c[:, 3] + 1.0) * (height / 2.0)
    return bool(np.any(np.abs(xs) > GUARD_PX) or np.any(np.abs(ys) > GUARD_PX))


class ClippedTri:
    """One triangle that goes through the clipper, by the definition of the clip volume.

    With v_i = (x, y, w)_i, D = det[v_0 v_1 v_2] and p^ = (ndc_x, ndc_y, 1) of a pixel centre, mu_i = det[p^, v_i+1,
    v_i+2] / D are the coordinates of p^ in the basis v_i: p^ = sum mu_i v_i, the ray through the pixel meets the
    triangle's plane at sum lambda_i (x, y, z, w)_i with lambda_i = mu_i / sum mu, and there w_p = 1 / sum mu and
    z_p = sum mu_i z_i / sum mu.  The point lies in the triangle and in front of the eye iff every mu_i >= 0 (all <= 0 is
    the image of what lies behind the eye), and inside the clip volume iff 0 <= z_p <= w_p, which is 0 <= sum mu_i z_i
    <= 1.  The x and y planes are the target's border and decide no pixel centre.  So the covered set is where five
    functions, each AFFINE in the window position, are >= 0:
        g_0..2 = mu_i,   g_3 = sum mu_i z_i (z >= 0),   g_4 = 1 - sum mu_i z_i (z <= w).
    Values: depth = z_p / w_p = g_3;  q = 1 / w_p = sum mu_i;  r = 1 / q;  a = sum mu_i a_i / q.

    THE BAND.  s_j = g_j / |grad g_j| (gradient per pixel) is the signed distance of a pixel centre from the line
    g_j = 0.  With m = min_j s_j a pixel is ideally covered iff m >= 0; a covered centre with m > tau is farther than
    tau from every boundary, an uncovered one with m < -tau is farther than tau outside one; |m| <= tau is offered either
    way (which keeps to the part of each line that bounds the kept region, up to tau at its corners).
    tau = sqrt(2)/512 + F:
      * each end of a piece's edge is a snapped point, at most 1/512 px from the clipper's fp32 vertex in x and in y:
        sqrt(2)/512 px; between its ends a line moves by no more than its ends do;
      * F, the fp32 error of the clipper's vertex in pixels.  One cut: t = d_in / (d_in - d_out) has the roundings of
        d_in, d_out (w - z, w +- x: one each), of the difference (no cancellation: the terms have the same sign) and of
        the quotient, 4 eps t;  k' = fma(t, out_k - in_k, in_k) adds eps t |out_k - in_k| for the difference and eps |k'|
        for the fma.  Together (4 + 1) eps |k' - in_k| + eps |k'| <= 11 eps max(|k'|, |in_k|) per component.  The z
        planes come first: their new vertices may lie as far out as the parent's, |component| <= M_z, the largest over
        the corners of (triangle and 0 <= z <= w), and a vertex passes at most both: 2 * 11 eps M_z, nothing where no
        vertex is beyond a z plane.  An x or y plane cuts at a kept magnitude: the new vertex has |x|, |y|, z <= w <=
        M_kept, and an error e <= 11 eps |P| made at a far end P of the cut edge reaches it scaled by the lever
        |k' - in| / |P - in| <= 2 M_kept / |P|; two such planes per vertex: 2 * 2 * 11 eps M_kept.  Then C3: x_s =
        (x / w + 1) W/2 carries a clip error e_x, e_w as (W/2) (e_x + |x/w| e_w) / w <= (W/2) 2 e / w_min with w_min the
        smallest w of the kept region, and C3's own three roundings, 4 eps W, on top.
    The corners of the kept region and of (triangle and the z planes) are found as what they are, the extreme points of
    the set that the inequalities describe (every pair of bounding lines intersected, the feasible points kept), in
    float64; they feed M_z, M_kept, w_min and the magnitudes of the allowances only, never a value or the coverage.
    (Over family D tau runs from 0.0029 to 0.0057 px; the oracle's worst coverage disagreement lies 0.0017 px from the
    ideal boundary, the HIP library's the same: DESIGN.md section 2.)

    ALLOWANCES.  For a quantity f that a piece interpolates screen-linearly (z_s, q = 1/w, a' = a/w) from its vertices:
      fp32, as `_chain`: <= 12 eps (|f_0| + |b1| (|f_1| + |f_0|) + |b2| (|f_2| + |f_0|)) <= 12 eps * 3 A_f inside the piece
        (b1 + b2 <= 1), A_f the largest |f| over the corners of the kept region.  Magnitude sum 3 A_f.
      cut-vertex term: a cut vertex's component k carries the 11 eps above less the 4 eps |k' - in_k| of t, which slides
        the vertex along its edge with every component in step and so leaves the interpolated function alone: <= 7 eps
        M_k per plane passed, M_k the largest |component| among the parent's vertices (every vertex the clipper makes
        is a convex combination of them); three planes counted as for F (both z planes, and x/y at kept magnitudes
        <= M_k): e_k = 7 eps * 3 M_k.  Through the partial derivatives of k / w:  z_s: (e_z + e_w) / w_min;  q: e_w /
        w_min^2;  a': e_a / w_min + M_a e_w / w_min^2.  Magnitude sum: the same with 3 M_k in place of e_k.
      snap term (listed separately, `snap`): moving a piece's vertices by at most S = 1/512 + F per axis with their
        attributes kept transports the interpolated function by at most that, for the rational u, v too (numerator and
        denominator move together): (|df/dx| + |df/dy|) S, gradients per pixel.
    r, u, v then follow from q and a' as in `Tri.attributes`.  b1, b2 are a piece's and are not the reference's to state."""

    PLANES = 3  # per cut vertex, in the cut-vertex term

    def __init__(self, clip, uv, width, height, bounds=True):
        """bounds=False: the ideal coverage and the distances only (no tau, no allowances)"""
        c = np.asarray(clip, dtype=np.float32).astype(np.float64)
        self.c, self.uv = c, np.asarray(uv, dtype=np.float32).astype(np.float64)
        self.width, self.height = width, height
        V = c[:, [0, 1, 3]]
        self.D = float(np.dot(V[0], np.cross(V[1], V[2])))
        self.empty = self.D == 0.0
        if self.empty:
            return
        # mu_i = p^ . N_i with N_i = (v_i+1 x v_i+2) / D; rows (a, b, c) of a ndc_x + b ndc_y + c
        N = np.array([np.cross(V[(i + 1) % 3], V[(i + 2) % 3]) for i in range(3)]) / self.D
        self.N = N
        z = c[:, 2]
        G = [N[0], N[1], N[2], z @ N, np.array([0.0, 0.0, 1.0]) - z @ N]
        if is_wrong("no_far"):
            G[3] = np.array([0.0, 0.0, 1.0])
        if is_wrong("no_near"):
            G[4] = np.array([0.0, 0.0, 1.0])
        self.G = np.array(G)
        if bounds:
            self._corners()

    # -- affine functions of the window position: f(px, py) = A px + B py + C at pixel centre (px + 1/2, py + 1/2)
    def _affine(self, row):
        a, b, c = row
        A, B = 2.0 * a / self.width, 2.0 * b / self.height
        return A, B, c - a - b + 0.5 * A + 0.5 * B

    def _eval(self, row, px, py):
        A, B, C = self._affine(row)
        return A * px + B * py + C

    def _corners(self):
        """extreme points (as barycentric lambda) of the kept region and of (triangle and the z planes); the bounds"""
        c = self.c
        lam_rows = [np.array(r, np.float64) for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]  # lambda_i >= 0
        zrows = [c[:, 3] - c[:, 2], c[:, 2]]                                              # w - z >= 0, z >= 0
        zrows = [r for r, dropped in zip(zrows, ("no_near", "no_far")) if not is_wrong(dropped)]
        xyrows = [c[:, 3] + c[:, 0], c[:, 3] - c[:, 0], c[:, 3] + c[:, 1], c[:, 3] - c[:, 1]]

        def extreme(rows):
            scale = [max(np.abs(r).max(), 1e-300) for r in rows]
            pts = []
            for i in range(len(rows)):
                for j in range(i + 1, len(rows)):
                    Mx = np.array([rows[i], rows[j], np.ones(3)])
                    if abs(np.linalg.det(Mx)) < 1e-12 * scale[i] * scale[j]:
                        continue
                    lam = np.linalg.solve(Mx, np.array([0.0, 0.0, 1.0]))
                    if all(float(r @ lam) >= -1e-9 * s * max(1.0, np.abs(lam).max()) for r, s in zip(rows, scale)):
                        pts.append(lam)
            return np.array(pts).reshape(-1, 3)

        zcross = bool(np.any(c[:, 2] < 0) or np.any(c[:, 2] > c[:, 3]))
        kept = extreme(lam_rows + zrows + xyrows)
        self.kept = kept @ c if len(kept) else np.zeros((0, 4))  # clip coordinates of the kept region's corners
        if len(kept) < 3 or self.kept[:, 3].max() <= 0.0:
            self.empty = True
            return
        self.kept_uv = kept @ self.uv
        pos = self.kept[:, 3] > 0
        self.w_min = float(self.kept[pos, 3].min())
        m_kept = float(np.abs(self.kept).max())
        m_z = float(np.abs(extreme(lam_rows + zrows) @ c).max()) if zcross else 0.0
        e_clip = 11.0 * EPS * (2.0 * m_z + 4.0 * m_kept)
        self.F = max(self.width, self.height) / 2.0 * 2.0 * e_clip / self.w_min + 4.0 * EPS * max(self.width, self.height)
        self.tau = math.sqrt(2.0) / 512.0 + self.F
        self.S = 1.0 / 512.0 + self.F
        self.M = np.abs(c).max(axis=0)      # per component, the parent's vertices
        self.M_uv = np.abs(self.uv).max(axis=0)

    def signed_distance(self, skip=()):
        """min_j s_j over the target (height, width); rows in `skip` left out"""
        py, px = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
        m = np.full((self.height, self.width), np.inf)
        for j, row in enumerate(self.G):
            if j in skip:
                continue
            A, B, C = self._affine(row)
            g, norm = A * px + B * py + C, math.hypot(A, B)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = g / norm if norm > 0 else np.where(g > 0, np.inf, np.where(g < 0, -np.inf, 0.0))
            m = np.minimum(m, s)
        return m

    def coverage(self):
        if self.empty:
            return np.zeros((self.height, self.width), bool)
        m = self.signed_distance()
        cov = m >= 0.0
        if is_wrong("behind_the_eye"):
            py, px = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
            cov |= np.all([self._eval(self.N[i], px, py) <= 0.0 for i in range(3)], axis=0)
        return cov

    def offered(self):
        if self.empty:
            return np.zeros((self.height, self.width), bool)
        return np.abs(self.signed_distance()) <= self.tau

    def attributes(self, px, py):
        px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
        z, w = self.c[:, 2], self.c[:, 3]
        Sx = self.S
        e, L = 7.0 * EPS, float(self.PLANES)  # cut-vertex term: per unit of its magnitude sum, planes counted
        wm = self.w_min
        zero = np.zeros(len(px))
        out = {"b1": (zero, zero + np.inf, zero), "b2": (zero, zero + np.inf, zero)}
        snap = {}

        def lin(row, A_f, cut_mag):
            A, B, _ = self._affine(row)
            val = self._eval(row, px, py)
            mag = 3.0 * A_f + cut_mag + 0.0 * val
            return val, 12.0 * EPS * 3.0 * A_f + e * cut_mag + 0.0 * val, mag, (abs(A) + abs(B)) * Sx, (A, B)

        # depth = z_s: |z_s| <= 1 over the clip volume
        d, dd, md, sd, _ = lin(z @ self.N, float(np.abs(self.kept[:, 2] / np.where(self.kept[:, 3] > 0, self.kept[:, 3], 1.0)).max()),
                               L * (self.M[2] + self.M[3]) / wm)
        out["depth"], snap["depth"] = (np.clip(d, 0.0, 1.0), dd + sd, md), sd
        q, dq, mq, _, gq = lin(self.N.sum(axis=0), 1.0 / wm, L * self.M[3] / wm ** 2)
        r = 1.0 / q
        sr = (abs(gq[0]) + abs(gq[1])) / q ** 2 * Sx
        out["r"], snap["r"] = (r, dq / q ** 2 + 2 * EPS / np.abs(q) + sr, mq / q ** 2), sr
        for k, name in enumerate("uv"):
            a = self.uv[:, k]
            A_n = float(np.abs(self.kept_uv[:, k] / np.where(self.kept[:, 3] > 0, self.kept[:, 3], np.inf)).max())
            num, dn, mn, _, gn = lin(a @ self.N, A_n, L * (self.M_uv[k] / wm + self.M_uv[k] * self.M[3] / wm ** 2))
            val = num / q
            if is_wrong("affine_uv"):  # mu_i w_i sum to 1: the weights of screen-linear interpolation
                val = sum(self._eval(self.N[i], px, py) * w[i] * a[i] for i in range(3))
            su = (np.abs((gn[0] - val * gq[0]) / q) + np.abs((gn[1] - val * gq[1]) / q)) * Sx
            out[name] = (val, dn / np.abs(q) + np.abs(val) * dq / np.abs(q) + 3 * EPS * np.abs(val) + su,
                         mn / np.abs(q) + np.abs(val) * mq / np.abs(q))
            snap[name] = su
        out["snap"] = snap
        return out


# ---------------------------------------------------------------- texel filtering
def level_extent(n, level):
    return max(1, n >> level) if not is_wrong("ceil_extent") else max(1, -(-n // (1 << level)))


def _wrap(i, n):
    """REPEAT: i mod size"""
    return np.mod(i, n) if not is_wrong("fmod_wrap") else np.maximum(np.fmod(i, n), 0)


def _fetch(img, i, j):
    """UNORM8 -> c / 255; indices beyond the stored level (only a wrong variant makes them) read its last texel"""
    return img[np.minimum(j, img.shape[0] - 1), np.minimum(i, img.shape[1] - 1)].astype(np.float64) / 255.0


def sample_level(img, wl, hl, filt, u, v, du, dv, su, sv):
    """One level at unnormalised U = u wl, V = v hl.  -> value (n, 4), allowance (n, 4), near-a-jump (n,) bool.
    dU = wl du + eps (|frac U| wl + 1): the contract forms (u - floor u) * wl, one rounding, and U - 1/2.
    NEAREST: texel floor(U).  The choice jumps where U is within dU of an integer: `near`; su, sv = -1 / +1 pick the
      texel on either side there.  Allowance: 4 eps (the conversion c * fl(1/255)).
    LINEAR: taps floor(U - 1/2), + 1 with weight frac(U - 1/2), likewise in V.  Continuous in U and V, so the allowance
      is (dU + dV) times the largest difference among the taps the footprint can reach (the 2x2 taps, and the next row or
      column where U - 1/2 is within dU of an integer), + 4 eps for the filter's own roundings (values <= 1)."""
    n = len(u)
    U, V = u * wl, v * hl
    dU = wl * du + EPS * (wl + 1.0)
    dV = hl * dv + EPS * (hl + 1.0)
    # NEAREST
    near = (np.floor(U - dU) != np.floor(U + dU)) | (np.floor(V - dV) != np.floor(V + dV))
    i = _wrap(np.floor(U + su * dU).astype(np.int64), wl)
    j = _wrap(np.floor(V + sv * dV).astype(np.int64), hl)
    val_n = _fetch(img, i, j)
    tol_n = np.full((n, 4), 4 * EPS)
    # LINEAR
    Uh, Vh = (U - 0.5, V - 0.5) if not is_wrong("taps_floor_u") else (U, V)
    i0, j0 = np.floor(Uh).astype(np.int64), np.floor(Vh).astype(np.int64)
    al, be = (Uh - i0)[:, None], (Vh - j0)[:, None]
    t = [[_fetch(img, _wrap(i0 + a, wl), _wrap(j0 + b, hl)) for a in (-1, 0, 1, 2)] for b in (-1, 0, 1, 2)]  # t[row][column]
    val_l = (1 - be) * ((1 - al) * t[1][1] + al * t[1][2]) + be * ((1 - al) * t[2][1] + al * t[2][2])
    use_c = [np.floor(Uh - dU) < i0, np.ones(n, bool), np.ones(n, bool), np.floor(Uh + dU) > i0]
    use_r = [np.floor(Vh - dV) < j0, np.ones(n, bool), np.ones(n, bool), np.floor(Vh + dV) > j0]
    hi, lo = np.full((n, 4), -np.inf), np.full((n, 4), np.inf)
    for b in range(4):
        for a in range(4):
            m = (use_r[b] & use_c[a])[:, None]
            hi = np.where(m, np.maximum(hi, t[b][a]), hi)
            lo = np.where(m, np.minimum(lo, t[b][a]), lo)
    tol_l = (dU + dV)[:, None] * (hi - lo) + 4 * EPS
    lin = (filt == LINEAR)[:, None]
    return np.where(lin, val_l, val_n), np.where(lin, tol_l, tol_n), near & (filt == NEAREST)


def sample(mips, smp, u, v, du, dv, lam, dlam, su=0.0, sv=0.0):
    """The texel at LOD lam (already clamped), whose own uncertainty after the clamp is dlam.
    smp = (mag, min, mip mode, min_lod, max_lod).  -> value, allowance, near-a-NEAREST-jump.
    Mag filter if lam <= 0, else min.  Mip NEAREST: level ceil(lam + 1/2) - 1, clamped to [0, q].  Mip LINEAR: levels
    floor(lc) and + 1 of lc = clamp(lam, 0, q), blended by frac(lc): continuous in lam, so its allowance is the levels'
    own, blended, + |lo - hi| dlam (the steepest of the level pairs lam +- dlam reaches) + 4 eps."""
    mag, minf, mip = smp[:3]
    q = len(mips) - 1
    w0, h0 = mips[0].shape[1], mips[0].shape[0]
    mag_min = (mag, minf) if not is_wrong("mag_min_swapped") else (minf, mag)
    filt = np.where(lam <= 0.0, mag_min[0], mag_min[1])
    L = [sample_level(mips[l], level_extent(w0, l), level_extent(h0, l), filt, u, v, du, dv, su, sv) for l in range(q + 1)]
    val_all = np.stack([x[0] for x in L])
    tol_all = np.stack([x[1] for x in L])
    near_all = np.stack([x[2] for x in L])
    idx = np.arange(len(u))
    if mip == NEAREST:
        d = np.ceil(lam + 0.5) - 1 if not is_wrong("floor_lambda") else np.floor(lam)
        d = np.clip(d, 0, q).astype(np.int64)
        return val_all[d, idx], tol_all[d, idx], near_all[d, idx]
    lc = np.clip(lam, 0.0, q)
    dhi = np.minimum(np.floor(lc).astype(np.int64), q)
    dlo = np.minimum(dhi + 1, q)
    delta = (lc - dhi)[:, None]
    hi, lo = val_all[dhi, idx], val_all[dlo, idx]
    val = hi + delta * (lo - hi)
    slope = np.abs(lo - hi)
    for k in range(q):  # a level pair next to this one that lam +- dlam reaches
        reach = ((np.floor(np.clip(lam - dlam, 0.0, q)) <= k) & (k <= np.floor(np.clip(lam + dlam, 0.0, q))))[:, None]
        slope = np.where(reach, np.maximum(slope, np.abs(val_all[k + 1] - val_all[k])), slope)
    tol = (1 - delta) * tol_all[dhi, idx] + delta * tol_all[dlo, idx] + slope * dlam[:, None] + 4 * EPS
    return val, tol, near_all[dhi, idx] | (near_all[dlo, idx] & (delta[:, 0] > 0))


# ---------------------------------------------------------------- a whole pass
class Ref:
    """What one pass must leave at every covered pixel (arrays over the covered pixels ys, xs in row-major order):
    val[name], tol[name], mag[name] for b1, b2, r, depth, u, v, deriv (n, 4: dudx, dvdx, dudy, dvdy), lam and texel
    (n, 4).  alts[k] lists the admissible (texel, allowance) pairs of covered pixel k where a discontinuous rule is
    within its allowance of the jump (the either/or rule); ambiguous marks those pixels.
    For triangles that went through the clipper: `clipped` marks their covered pixels, `snap[name]` is the part of
    tol[name] that is the snap term, and over the target (height, width) `offered` marks the pixels within tau of an ideal
    boundary, which may be covered or not, `dist` is every pixel's distance from the nearest such boundary and `tau` the
    widest band.  No other triangle has any of this: offered is all False and tau 0."""


def render(tris, width, height, mips, smp, exact=False):
    """tris: [(clip (3, 4) float32, uv (3, 2) float32)], drawn opaque in one pass; their coverage must be disjoint (the
    cases draw single triangles and pairs that share an edge).  A triangle that C2 routes through the clipper is a
    `ClippedTri`, every other a `Tri` on the exact path.  exact=True: the case is built so that both precisions
    compute the same lambda and the same texel coordinates; the jump bands are then zero and no either/or is offered."""
    T = [(ClippedTri if routed_to_clipper(c, width, height) else Tri)(c, t, width, height) for c, t in tris]
    owner = np.full((height, width), -1, np.int64)
    ref = Ref()
    # clipped triangles: the pixels offered either way, their distance from the ideal boundary, the widest band
    ref.offered, ref.dist, ref.tau = np.zeros((height, width), bool), np.full((height, width), np.inf), 0.0
    for k, t in enumerate(T):
        c = t.coverage()
        assert not (c & (owner >= 0)).any(), "the reference draws disjoint triangles only"
        owner[c] = k
        if isinstance(t, ClippedTri) and not t.empty:
            ref.offered |= t.offered()
            ref.dist = np.minimum(ref.dist, np.abs(t.signed_distance()))
            ref.tau = max(ref.tau, t.tau)
    ref.tris, ref.covered = T, owner >= 0
    ref.ys, ref.xs = np.nonzero(ref.covered)
    n = len(ref.ys)
    ref.clipped = np.array([isinstance(T[k], ClippedTri) for k in owner[ref.ys, ref.xs]], bool)
    names = ("b1", "b2", "r", "depth", "u", "v")
    ref.val = {k: np.zeros(n) for k in names}
    ref.tol = {k: np.zeros(n) for k in names}
    ref.mag = {k: np.zeros(n) for k in names}
    ref.snap = {k: np.zeros(n) for k in names}  # the part of tol that is the snap term (clipped triangles only)
    deriv, dderiv, sderiv = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4))
    for k, t in enumerate(T):
        m = owner[ref.ys, ref.xs] == k
        if not m.any():
            continue
        px, py = ref.xs[m], ref.ys[m]
        here = t.attributes(px, py)
        for name in names:
            ref.val[name][m], ref.tol[name][m], ref.mag[name][m] = here[name]
            ref.snap[name][m] = here.get("snap", {}).get(name, 0.0)
        # derivatives: the pixel's own triangle at its partners in the 2x2 quad (aligned to even coordinates), forward
        # differences; each is a difference of two interpolated values: d = du_a + du_b + 2 eps |difference|
        horiz, vert = t.attributes(px ^ 1, py), t.attributes(px, py ^ 1)
        sx, sy = np.where(px & 1, -1.0, 1.0), np.where(py & 1, -1.0, 1.0)
        for c, (part, sign, name) in enumerate(((horiz, sx, "u"), (horiz, sx, "v"), (vert, sy, "u"), (vert, sy, "v"))):
            dm = sign * (part[name][0] - here[name][0])
            deriv[m, c] = dm
            dderiv[m, c] = part[name][1] + here[name][1] + 2 * EPS * np.abs(dm)
            sderiv[m, c] = part.get("snap", {}).get(name, 0.0) + here.get("snap", {}).get(name, 0.0)
    ref.snap["deriv"] = sderiv
    ref.val["deriv"], ref.tol["deriv"] = deriv, dderiv
    # lambda = log2(rho), rho the longer of the two derivative vectors scaled by the level-0 extent.
    #   m = d * W0: one rounding            dm = W0 dd + eps |m|
    #   rho^2 = mx^2 + my^2: two roundings  d(rho^2) = 2 |mx| dmx + 2 |my| dmy + 3 eps rho^2
    #   lambda = log2(rho^2) / 2            dlam = d(rho^2) / (2 ln2 rho^2) + 5e-5 (the polynomial, C8)
    w0, h0 = mips[0].shape[1], mips[0].shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        lam_ax, dlam_ax = [], []
        for c in (0, 2):
            mx, my = deriv[:, c] * w0, deriv[:, c + 1] * h0
            dmx, dmy = w0 * dderiv[:, c] + EPS * np.abs(mx), h0 * dderiv[:, c + 1] + EPS * np.abs(my)
            rho2 = mx * mx + my * my
            lam_ax.append(0.5 * np.log2(rho2))
            # (constant uv: rho = 0, lambda = -inf, which every clamp decides)
            dlam_ax.append(np.where(rho2 > 0, (2 * np.abs(mx) * dmx + 2 * np.abs(my) * dmy + 3 * EPS * rho2) / (2 * math.log(2.0) * rho2), 0.0))
        lam = np.maximum(lam_ax[0], lam_ax[1])
        # the larger axis's error where it leads by more than both errors, else the larger error
        lead0 = lam_ax[0] - dlam_ax[0] > lam_ax[1] + dlam_ax[1]
        lead1 = lam_ax[1] - dlam_ax[1] > lam_ax[0] + dlam_ax[0]
        dlam = np.where(lead0, dlam_ax[0], np.where(lead1, dlam_ax[1], np.maximum(dlam_ax[0], dlam_ax[1]))) + LOD_POLY
    ref.val["lam"], ref.tol["lam"] = lam, dlam
    band = 0.0 if exact else 1.0
    lo = np.clip(lam - band * dlam, smp[3], smp[4])
    hi = np.clip(lam + band * dlam, smp[3], smp[4])
    mid = np.clip(lam, smp[3], smp[4])
    dmid = np.maximum(hi - mid, mid - lo)  # what is left of dlam after the clamp: none where the clamp decides
    u, v, du, dv = ref.val["u"], ref.val["v"], ref.tol["u"] * band, ref.tol["v"] * band
    val, tol, near = sample(mips, smp, u, v, du, dv, mid, dmid)
    if exact:  # the allowance of the value keeps u's own error
        tol = sample(mips, smp, u, v, ref.tol["u"], ref.tol["v"], mid, dmid)[1]
    ref.val["texel"], ref.tol["texel"] = val, tol
    q = len(mips) - 1
    jump = near.copy()
    if smp[0] != smp[1]:
        jump |= (lo <= 0.0) & (hi > 0.0)
    if smp[2] == NEAREST:
        jump |= np.clip(np.ceil(lo + 0.5) - 1, 0, q) != np.clip(np.ceil(hi + 0.5) - 1, 0, q)
    ref.ambiguous = jump
    ref.alts = {}
    k = np.nonzero(jump)[0]
    if len(k):
        cands = []
        for lam_end in (lo[k], hi[k]):
            for su in (-1.0, 1.0):
                for sv in (-1.0, 1.0):
                    cands.append(sample(mips, smp, u[k], v[k], du[k], dv[k], lam_end, dmid[k] * 0.0 + (hi[k] - lo[k]), su, sv)[:2])
        for row, pix in enumerate(k):
            ref.alts[int(pix)] = [(c[0][row], c[1][row]) for c in cands]
    return ref
