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
reference."""
import math

import numpy as np

EPS = 2.0 ** -24
LOD_POLY = 5e-5  # DESIGN C8: the stated error of the log2 polynomial
NEAREST, LINEAR = 0, 1
WRONG = None
VARIANTS = ("bottom_right", "affine_uv", "taps_floor_u", "floor_lambda", "ceil_extent", "fmod_wrap", "mag_min_swapped")


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
    within its allowance of the jump (the either/or rule); ambiguous marks those pixels."""


def render(tris, width, height, mips, smp, exact=False):
    """tris: [(clip (3, 4) float32, uv (3, 2) float32)], drawn opaque in one pass; their coverage must be disjoint (the
    cases draw single triangles and pairs that share an edge).  exact=True: the case is built so that both precisions
    compute the same lambda and the same texel coordinates; the jump bands are then zero and no either/or is offered."""
    T = [Tri(c, t, width, height) for c, t in tris]
    owner = np.full((height, width), -1, np.int64)
    for k, t in enumerate(T):
        c = t.coverage()
        assert not (c & (owner >= 0)).any(), "the reference draws disjoint triangles only"
        owner[c] = k
    ref = Ref()
    ref.tris, ref.covered = T, owner >= 0
    ref.ys, ref.xs = np.nonzero(ref.covered)
    n = len(ref.ys)
    names = ("b1", "b2", "r", "depth", "u", "v")
    ref.val = {k: np.zeros(n) for k in names}
    ref.tol = {k: np.zeros(n) for k in names}
    ref.mag = {k: np.zeros(n) for k in names}
    deriv, dderiv = np.zeros((n, 4)), np.zeros((n, 4))
    for k, t in enumerate(T):
        m = owner[ref.ys, ref.xs] == k
        px, py = ref.xs[m], ref.ys[m]
        here = t.attributes(px, py)
        for name in names:
            ref.val[name][m], ref.tol[name][m], ref.mag[name][m] = here[name]
        # derivatives: the pixel's own triangle at its partners in the 2x2 quad (aligned to even coordinates), forward
        # differences; each is a difference of two interpolated values: d = du_a + du_b + 2 eps |difference|
        horiz, vert = t.attributes(px ^ 1, py), t.attributes(px, py ^ 1)
        sx, sy = np.where(px & 1, -1.0, 1.0), np.where(py & 1, -1.0, 1.0)
        for c, (part, sign, name) in enumerate(((horiz, sx, "u"), (horiz, sx, "v"), (vert, sy, "u"), (vert, sy, "v"))):
            dm = sign * (part[name][0] - here[name][0])
            deriv[m, c] = dm
            dderiv[m, c] = part[name][1] + here[name][1] + 2 * EPS * np.abs(dm)
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
