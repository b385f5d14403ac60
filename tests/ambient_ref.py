"""Test-side helpers of the ambient pass (include/svr_ambient.h): build and run tests/native/ambient_ref.cpp, the scalar
restatement of DESIGN C32-C37 (and of C17-C19 with the ambient factor); ao64, the same pass stated in float64 from the
definitions, with its ties and its derived bound (family O); and the inputs the tests share.  Depth
travels as float32 [H, W], the normal plane as float32 [H, W, 4], matrices as 4 x 4 indexed [col][row] like glmath's or as
16 floats, column-major."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import __graft_entry__ as g
import native_ref as N

pkg = g.load_package()
A, GL = pkg.abi, pkg.glmath
f32 = np.float32
NO_BLUR = 1
NO_SURFACE, SMALL, EVALUATED, CAPPED = 1, 2, 3, 4  # the reference's "kind" of a pixel inside the scissor


ref_exe = functools.partial(N.build, "ambient_ref", extra=("-Wall", "-Werror"))


def m16(m):
    return np.ascontiguousarray(np.asarray(m, dtype=f32).reshape(16))


def _run(mode, blob, size):
    raw = N.run(ref_exe(), blob, mode)
    assert len(raw) == size
    return raw


def frame_blob(depth, normal, inv_vp, radius, ppu, bias=0.0, intensity=1.0, sharpness=0.05, flags=0, scissor=None, variant=0):
    """the <in> of ambient_ref ao; variant: a wrong variant of one rule (WRONG_VARIANTS), in bits 16-23 of the flags word"""
    depth = np.ascontiguousarray(depth, dtype=f32)
    h, w = depth.shape
    normal = np.ascontiguousarray(normal, dtype=f32)
    assert normal.shape == (h, w, 4) and 0 <= flags < 1 << 16 and 0 <= variant < 256
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    return np.array([w, h, sx, sy, sw, sh, flags | variant << 16], np.uint32).tobytes() + m16(inv_vp).tobytes() + \
        np.array([radius, ppu, bias, intensity, sharpness], f32).tobytes() + depth.tobytes() + normal.tobytes()


def run_ref(depth, normal, inv_vp, radius, ppu, bias=0.0, intensity=1.0, sharpness=0.05, flags=0, scissor=None, variant=0, exe=None):
    """ambient_ref ao over one frame -> {"raw": f32 [H,W,2], "out": f32 [H,W], "kind": uint8 [H,W]}; zeros outside the scissor.
    exe: another build of ambient_ref.cpp (the sanitized one)"""
    h, w = np.shape(depth)
    blob = frame_blob(depth, normal, inv_vp, radius, ppu, bias, intensity, sharpness, flags, scissor, variant)
    n = w * h
    raw = _run("ao", blob, n * 13) if exe is None else N.run(exe, blob, "ao")
    assert len(raw) == n * 13
    return {"raw": np.frombuffer(raw, f32, n * 2, 0).reshape(h, w, 2).copy(),
            "out": np.frombuffer(raw, f32, n, n * 8).reshape(h, w).copy(),
            "kind": np.frombuffer(raw, np.uint8, n, n * 12).reshape(h, w).copy()}


def run_light_ref(depth, normal, albedo, ao, inv_vp, ambient, sun_dir, sun_color, lights=None):
    """ambient_ref light: lighting_ref.run_ref's result with the ambient term scaled by ao (no shadow map)"""
    h, w = depth.shape
    lights = np.zeros(0, A.POINT_LIGHT_DTYPE) if lights is None else np.ascontiguousarray(lights, dtype=A.POINT_LIGHT_DTYPE)
    parts = [np.array([w, h, lights.size, 0, 0], np.uint32).tobytes(), m16(inv_vp).tobytes()]
    parts += [np.asarray(v, f32).reshape(4).tobytes() for v in (ambient, sun_dir, sun_color)]
    parts += [np.zeros(17, f32).tobytes(), lights.tobytes()]
    parts += [np.ascontiguousarray(a, dtype=f32).tobytes() for a in (depth, normal, albedo, ao)]
    n = w * h
    raw = _run("light", b"".join(parts), n * 30)
    return {"rgba": np.frombuffer(raw, f32, n * 4, 0).reshape(h, w, 4).copy(),
            "winner": np.frombuffer(raw, np.uint8, n, n * 16).reshape(h, w).astype(bool),
            "position": np.frombuffer(raw, f32, n * 3, n * 17).reshape(h, w, 3).copy(),
            "shadowed": np.frombuffer(raw, np.uint8, n, n * 29).reshape(h, w).astype(bool)}


@functools.lru_cache(maxsize=None)
def tables():
    """(D f32 [8,2], R f32 [16,2], f f32 [8]): the kernel's tap tables and the radius fractions, as ambient_ref has them"""
    with tempfile.TemporaryDirectory(prefix="ambient_ref_io_") as d:
        fout = os.path.join(d, "tables.bin")
        subprocess.run([ref_exe(), "tables", fout], check=True)
        t = np.fromfile(fout, f32)
    assert t.size == 16 + 32 + 8
    return t[:16].reshape(8, 2), t[16:48].reshape(16, 2), t[48:]


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def assert_planes(got, want, what, mask=None):
    """bit patterns, every element (mask: [H, W] of the pixels that count)"""
    bad = bits(got) != bits(want)
    if bad.ndim == 3:
        bad = bad.any(axis=-1)
    if mask is not None:
        bad &= mask
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                             f"{np.asarray(got)[y, x].tolist()} vs {np.asarray(want)[y, x].tolist()}")


def inside_of(shape, scissor):
    m = np.zeros(shape, bool)
    x0, y0, sw, sh = scissor
    m[y0:y0 + sh, x0:x0 + sw] = True
    return m


# ---- the random planes of the GPU test (chosen and checked on the CPU: test_ambient_ref.py)
CAMERA = ((0.0, 2.0, 0.0), 0.1, 1.5)


def camera(w, h, cam=CAMERA):
    """(inv_viewproj as 16 floats, pixels_per_unit) of a real camera over a w x h target"""
    pos, pitch, yaw = cam
    view, proj, viewproj = GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[:3]
    m = np.asarray(viewproj, dtype=np.float64).reshape(4, 4).T
    return m16(np.linalg.inv(m).T), GL.pixels_per_unit(proj, h)


def random_gbuffer(w, h, seed, near=0.1):
    """depth float32 [h, w] and normal float32 [h, w, 4].  Depth: runs of equal values along a row, repeated over a few
    rows, whose clip w = near / depth is log-uniform over 0.3 .. 80 (reversed Z: depth = near / w), with steps between
    them, some ramps, and runs of exact 0.  Normals: random directions of random length; some texels are non-winners
    (all-zero bits) and some winners have a zero normal."""
    rng = np.random.default_rng(seed)
    z = np.zeros((h, w), f32)
    y = 0
    while y < h:
        rows = int(rng.integers(1, 7))
        x = 0
        while x < w:
            n = int(rng.integers(3, 28))
            wc = 10.0 ** rng.uniform(np.log10(0.3), np.log10(80.0))
            kind = rng.uniform()
            run = np.full((rows, n), near / wc)
            if kind < 0.12:
                run[:] = 0.0
            elif kind < 0.4:  # a ramp: a surface tilted against the view
                run = near / (wc * (1.0 + 0.02 * np.arange(n)[None, :] + 0.03 * np.arange(rows)[:, None]))
            z[y:y + rows, x:x + n] = run[:h - y, :w - x].astype(f32)
            x += n
        y += rows
    nrm = np.zeros((h, w, 4), f32)
    nrm[..., :3] = rng.normal(0, 1, (h, w, 3)).astype(f32) * rng.uniform(0.2, 2.0, (h, w, 1)).astype(f32)
    nrm[..., 3] = rng.uniform(0.1, 1.0, (h, w)).astype(f32)  # a winner's light term
    nrm[rng.uniform(size=(h, w)) < 0.04] = 0.0  # non-winners
    nrm[rng.uniform(size=(h, w)) < 0.03, :3] = 0.0  # winners with a zero normal
    return z, nrm


PLANE = (130, 67)  # 5 x 3 tiles of 32: both extents cross tile seams and end in a partial tile
ODD_SCISSOR = (3, 5, 117, 59)
# a radius whose rpx = radius * pixels_per_unit / w runs from below one pixel (w above 24) through the middle of the range to
# the cap of 16 (w below 1.5) over the planes' w of 0.3 .. 80
PLANE_PARAMS = dict(radius=0.5, bias=0.01, intensity=1.5, sharpness=0.05)


@functools.lru_cache(maxsize=None)
def plane_case(scissor, flags):
    """the random planes of the GPU test and the reference over them, computed once: (depth, normal, inv_viewproj, ppu, ref)"""
    w, h = PLANE
    inv_vp, ppu = camera(w, h)
    depth, normal = random_gbuffer(w, h, seed=81)
    ref = run_ref(depth, normal, inv_vp, ppu=ppu, flags=flags, scissor=scissor, **PLANE_PARAMS)
    return depth, normal, inv_vp, ppu, ref


def assert_plane_case_is_telling(ref, scissor):
    """the condition on the inputs, on the reference alone: a tenth of the scissor's pixels are darkened, a tenth are exactly
    1, and at least one pixel sits at the reach cap"""
    m = inside_of(ref["out"].shape, scissor or (0, 0) + PLANE)
    out = ref["out"][m]
    assert (out < 1).mean() >= 0.1 and (out == 1).mean() >= 0.1
    assert (ref["kind"][m] == CAPPED).any() and (ref["kind"][m] == SMALL).any() and (ref["kind"][m] == EVALUATED).any()
    assert (ref["kind"][m] == NO_SURFACE).any() and not ref["kind"][~m].any()


# ---------------------------------------------------------------- the fp64 statement, from the definitions
# C32-C37 a second time: numpy float64, written from include/svr_ambient.h and the contract's definitions, sharing none of
# ambient_ref.cpp's operation order and not reading csrc/svr_ambient_tables.h.  The fp32 depth plane, normal plane, matrix
# and parameters are taken as exact reals.
#
# ALLOWANCES follow light_geom_ref.py's and dof_ref.py's convention: EPS = 2^-24, first-order running forward bounds, every
# fp32 rounding of the contract's chain adds EPS times the magnitude of what it rounds, an input's error goes through the
# absolute partial derivative, and one further EPS |result| stands for the second-order terms.  Each derivation stands
# next to its line.  TIES: a pixel where one of the rule's jumps lies within its input's allowance (rpx at 1, a tap's
# rpx f_k u at a half-integer, a tap's v.v at radius^2, a blur tap's |hw_t - hw_c| at sharpness hw_c), and a pixel whose
# accepted blur taps include one, is left out of a comparison; nothing else is.  The cap at 16, max(v.n - bias, 0) and
# max(a, 0) are continuous: no rule there.
EPS = 2.0 ** -24
WRONG_VARIANTS = {1: "rotation indexed by scissor-relative coordinates", 2: "f_k from k instead of 3k & 7", 3: "rintf replaced by truncation",
                  4: "tap unprojected at the texel's corner", 5: "a tap outside the scissor clamped in", 6: "normal not normalised",
                  7: "bias added", 8: "range test dropped", 9: "blur clamped to the image", 10: "blur acceptance absolute",
                  11: "blur 3 x 3", 12: "the reach cap at 8"}


def tap_formulas():
    """C34 from its formulas, in float64: (angle [16, 8] in radians of tap k under rotation j, fraction [8])"""
    k, j = np.arange(8), np.arange(16)
    return np.radians(45.0 * k[None, :] + (45.0 / 16.0) * j[:, None]), (((3 * k) & 7) + 0.5) / 8.0


def matrix64(inv_vp):
    """column-major float[16] -> the float64 4 x 4 that multiplies column vectors"""
    return m16(inv_vp).astype(np.float64).reshape(4, 4).T


def unproject64(M, W, H, px, py, z):
    """C17 up to the divide, at the pixel centres: h = M (xn, yn, z, 1) [..., 4] and the first-order fp32 error of each
    component.  xn = (px + 0.5) (2 / W) - 1: the quotient is rounded once on the host and multiplies px + 0.5 = xn + 1, the
    fma rounds |xn| once.  A component of h is a product and three fmas: four roundings, none of more than the magnitude sum
    of its four terms; xn's and yn's errors come in through |m|.  z is the texel: exact."""
    xn, yn = (px + 0.5) * 2.0 / W - 1.0, (py + 0.5) * 2.0 / H - 1.0
    e_xn, e_yn = EPS * ((xn + 1.0) + np.abs(xn)), EPS * ((yn + 1.0) + np.abs(yn))
    terms = np.stack([M[:, 0] * xn[..., None], M[:, 1] * yn[..., None], M[:, 2] * z[..., None], M[:, 3] + 0.0 * z[..., None]])
    h, mag = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    e_h = np.abs(M[:, 0]) * e_xn[..., None] + np.abs(M[:, 1]) * e_yn[..., None] + 4.0 * EPS * mag
    return h, e_h


def divide64(h, e_h):
    """C17's divide: rw = 1 / h.w rounds once (d(1/w) = dw / w^2), p = h.xyz rw rounds once per component"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rw = 1.0 / h[..., 3]
        e_rw = e_h[..., 3] * rw * rw + EPS * np.abs(rw)
        p = h[..., :3] * rw[..., None]
        e_p = e_h[..., :3] * np.abs(rw)[..., None] + np.abs(h[..., :3]) * e_rw[..., None] + EPS * np.abs(p)
    return p, e_p


def ao64(depth, normal, inv_vp, radius, ppu, bias=0.0, intensity=1.0, sharpness=0.05, scissor=None, positions=None):
    """The ambient pass over the scissor in float64.  Returns planes of the target's extent, zero (False) outside the scissor:
    a, out: the factor before the store's rounding, without and with the blur; tie_a, tie_out: the pixels left out of a
    comparison of either; bound_a, bound_out: the first-order bound on |fp32 result - a| and |fp32 result - out|; hw: the
    raw plane's second component; rpx: the capped screen radius (0 without a surface).
    positions: float64 [H, W, 3], the surface points themselves (where the depth plane came from geometry): used for P and
    every Q instead of the unprojection.  The fp32 chain still unprojects the rounded texel, so its error is the chain's
    plus what the texel's rounding (half an ulp: EPS |z|) moves the point by along the ray, |dp/dz| = |M[:3, 2] - p M[3, 2]| / |h.w|."""
    depth = np.asarray(depth, dtype=f32)
    H, W = depth.shape
    sx, sy, sw, sh = scissor or (0, 0, W, H)
    box = (slice(sy, sy + sh), slice(sx, sx + sw))
    M = matrix64(inv_vp)
    radius, ppu, bias, intensity, sharpness = (float(f32(v)) for v in (radius, ppu, bias, intensity, sharpness))
    z = depth[box].astype(np.float64)
    nrm = np.asarray(normal, dtype=f32)[box]
    n3 = nrm[..., :3].astype(np.float64)
    y, x = np.mgrid[0:sh, 0:sw]
    px, py = x + sx, y + sy

    # C32: the centre.  In reals the squared length is > 0 iff a component is non-zero (the statement's inputs hold no
    # normal whose square underflows in fp32; tests/test_ambient_gpu.py's specials are the restatement's alone)
    h, e_h = unproject64(M, W, H, px, py, z)
    hw, e_hw = h[..., 3], e_h[..., 3]
    pos, e_pos = divide64(h, e_h)
    if positions is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            dpdz = np.abs(M[:3, 2] - pos * M[3, 2]) / np.abs(hw)[..., None]
        e_pos = e_pos + dpdz * (EPS * np.abs(z))[..., None]
        pos = np.asarray(positions, dtype=np.float64)[box]
    nn = (n3 * n3).sum(axis=-1)
    surface = (z > 0) & (nrm[..., 3].view(np.uint32) != 0) & (nn > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = n3 / np.sqrt(nn)[..., None]
    # nn: a product and two fmas of positive terms, 3 EPS nn; the root halves that and rounds, the reciprocal rounds, the
    # product rounds: 1.5 + 1 + 1 + 1
    e_nh = 4.5 * EPS * np.abs(nh)

    # C33: radius_px = radius ppu rounds once on the host, its product with h.w once
    rpx_raw = (radius * ppu) * hw
    e_rpx = (radius * ppu) * e_hw + 2.0 * EPS * np.abs(rpx_raw)
    tie_a = surface & (np.abs(rpx_raw - 1.0) <= e_rpx)
    evaluated = surface & (rpx_raw >= 1.0)
    rpx = np.minimum(rpx_raw, 16.0)
    e_rpx = np.where(rpx_raw > 16.0 + e_rpx, 0.0, e_rpx)  # at the cap whatever the roundings did: exactly 16

    # C34, C35
    angle, fraction = tap_formulas()
    rot = (py & 3) * 4 + (px & 3)
    total, e_total = np.zeros((sh, sw)), np.zeros((sh, sw))
    r2 = radius * radius
    c0 = float(f32(0.0001))
    for k in range(8):
        ux, uy = np.cos(angle[rot, k]), np.sin(angle[rot, k])
        # u = d R: the four literals are roundings of the formulas' values, each product rounds (3 EPS a product), and
        # the difference (the fma) rounds once
        dc, ds = np.cos(np.radians(45.0 * k)), np.sin(np.radians(45.0 * k))
        rc, rs = np.cos(np.radians(45.0 / 16.0 * rot)), np.sin(np.radians(45.0 / 16.0 * rot))
        e_ux = EPS * (3.0 * (np.abs(dc * rc) + np.abs(ds * rs)) + np.abs(ux))
        e_uy = EPS * (3.0 * (np.abs(dc * rs) + np.abs(ds * rc)) + np.abs(uy))
        rf = rpx * fraction[k]  # the fraction is an odd sixteenth: exact; the product rounds
        e_rf = fraction[k] * e_rpx + EPS * rf
        off = []
        for u, e_u in ((ux, e_ux), (uy, e_uy)):
            t = rf * u
            e_t = np.abs(u) * e_rf + rf * e_u + EPS * np.abs(t)
            with np.errstate(invalid="ignore"):
                tie_a |= evaluated & (np.abs(np.abs(t - np.floor(t)) - 0.5) <= e_t)
                off.append(np.where(evaluated, np.rint(t), 0.0).astype(np.int64))
        ox, oy = off
        tx, ty = x + ox, y + oy
        live = evaluated & ((ox != 0) | (oy != 0)) & (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        txc, tyc = np.clip(tx, 0, sw - 1), np.clip(ty, 0, sh - 1)
        live &= z[tyc, txc] > 0
        # Q is the tap's own position (C35): the same chain at its pixel centre and depth
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = pos[tyc, txc] - pos
            e_v = e_pos[tyc, txc] + e_pos + EPS * np.abs(v)  # the cancellation: two world magnitudes, a small difference
            vv = (v * v).sum(axis=-1)
            e_vv = (2.0 * np.abs(v) * e_v).sum(axis=-1) + 3.0 * EPS * vv  # a product and two fmas of positive terms
            tie_a |= live & (np.abs(vv - r2) <= e_vv + EPS * r2)  # radius^2 rounds once on the host
            live &= vv < r2
            dot, dot_mag = (v * nh).sum(axis=-1), np.abs(v * nh).sum(axis=-1)
            e_dot = (np.abs(nh) * e_v + np.abs(v) * e_nh).sum(axis=-1) + 3.0 * EPS * dot_mag
            vn = dot - bias
            e_vn = e_dot + EPS * np.abs(vn)
            den = vv + c0
            e_den = e_vv + EPS * den
            c = np.maximum(vn, 0.0) / den
            # max(., 0) widens nothing; below -e_vn the fp32 value is not positive either
            e_c = np.where(vn > -e_vn, e_vn / den + c * e_den / den + EPS * c, 0.0)
        total += np.where(live, c, 0.0)
        e_total += np.where(live, e_c, 0.0)
    e_total += 8.0 * EPS * total  # eight additions of non-negative terms, none of more than the final sum
    # C36: the coefficient (intensity radius) 0.125 rounds once; its product with the sum and the difference round
    coef = intensity * radius * 0.125
    au = 1.0 - coef * total
    e_a = coef * e_total + 2.0 * EPS * coef * total + EPS * np.abs(au)
    a = np.where(evaluated, np.maximum(au, 0.0), 1.0)
    e_a = np.where(evaluated, e_a, 0.0)
    tie_a &= surface
    hwr, e_hwr = np.where(surface, hw, 0.0), np.where(surface, e_hw, 0.0)  # the raw plane's (a, 1/w)

    # C37: 25 additions, none of more than the final sum, and the quotient
    acc, e_acc, count = np.zeros((sh, sw)), np.zeros((sh, sw)), np.zeros((sh, sw))
    tie_out = np.zeros((sh, sw), bool)
    centre = hwr != 0.0
    lim = sharpness * hwr
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ty, tx = np.clip(y + dy, 0, sh - 1), np.clip(x + dx, 0, sw - 1)
            d = np.abs(hwr[ty, tx] - hwr)
            if dx == 0 and dy == 0:
                accept = np.ones((sh, sw), bool)
            else:
                accept = d <= lim
                e_d = e_hwr[ty, tx] + e_hwr + EPS * d + sharpness * e_hwr + EPS * np.abs(lim)
                tie_out |= np.abs(d - lim) <= e_d
            tie_out |= accept & tie_a[ty, tx]
            acc += np.where(accept, a[ty, tx], 0.0)
            e_acc += np.where(accept, e_a[ty, tx], 0.0)
            count += accept
    out = np.where(centre, acc / count, 1.0)
    e_out = np.where(centre, (e_acc + 25.0 * EPS * acc) / count + EPS * out, 0.0)
    tie_out &= centre

    def plane(v, dtype=np.float64):
        full = np.zeros((H, W), dtype)
        full[box] = v
        return full
    return {"a": plane(a), "out": plane(out), "tie_a": plane(tie_a, bool), "tie_out": plane(tie_out, bool),
            "bound_a": plane(e_a + EPS * a), "bound_out": plane(e_out + EPS * out), "hw": plane(hwr),
            "rpx": plane(np.where(surface, rpx, 0.0))}


def view_of(st, flags):
    """(value, tie, bound) of a statement as the pass under flags stores it"""
    return (st["a"], st["tie_a"], st["bound_a"]) if flags & NO_BLUR else (st["out"], st["tie_out"], st["bound_out"])


TIE_CAP, DARK_SHARE, OPEN_SHARE = 0.02, 0.1, 0.1


def assert_statement_is_telling(st, flags, scissor):
    """the condition on the inputs, on the statement alone: at most 2 % of the scissor's pixels are ties, a tenth of the
    compared pixels are darkened and a tenth are exactly 1"""
    value, tie, _ = view_of(st, flags)
    m = inside_of(value.shape, scissor)
    keep = m & ~tie
    assert tie[m].mean() <= TIE_CAP, f"tie share {tie[m].mean():.4f}"
    assert (value[keep] < 1).mean() >= DARK_SHARE and (value[keep] == 1).mean() >= OPEN_SHARE, \
        f"darkened {(value[keep] < 1).mean():.3f}, open {(value[keep] == 1).mean():.3f}"


def compare64(got, st, flags, scissor):
    """an fp32 plane against the statement over the scissor's compared pixels -> (largest |got - statement| / bound, its
    (y, x), the number of compared pixels beyond the bound)"""
    value, tie, bound = view_of(st, flags)
    keep = inside_of(value.shape, scissor) & ~tie
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(keep, np.abs(np.asarray(got, dtype=np.float64) - value) / bound, 0.0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), (int(at[0]), int(at[1])), int((ratio > 1.0).sum())


@functools.lru_cache(maxsize=None)
def plane_statement(scissor):
    """ao64 over the random planes under a scissor, computed once"""
    depth, normal, inv_vp, ppu, _ = plane_case(scissor, 0)
    return ao64(depth, normal, inv_vp, ppu=ppu, scissor=scissor, **PLANE_PARAMS)


# ---------------------------------------------------------------- analytic scenes: depth and normals from geometry
SCENE = (96, 64)
SCENE_CAMERA = ((0.0, 1.0, 0.0), -0.3, 1.5)  # one unit over the floor, looking along +x and down: the floor starts at w of about 1
SCENE_PARAMS = dict(radius=1.0, bias=0.01, intensity=1.5, sharpness=0.05)  # rpx = 16 below w = 2.86, below one pixel above w = 45.7


def _box(centre, half, turn):
    """the five visible faces of a box standing on the floor, turned about y: [(normal, offset)] with n . X <= offset inside"""
    c, s = np.cos(turn), np.sin(turn)
    ax, az = np.array([c, 0.0, s]), np.array([-s, 0.0, c])
    cx = np.array([centre[0], 0.0, centre[1]])
    faces = [(sgn * a, float(sgn * a @ cx) + hlf) for a, hlf in ((ax, half[0]), (az, half[2])) for sgn in (1.0, -1.0)]
    return faces + [(np.array([0.0, 1.0, 0.0]), float(half[1]))]


BOX_TOP = 0.5
# convex solids as lists of half-spaces; the floor is the half-space y <= 0
FLOOR = [(np.array([0.0, 1.0, 0.0]), 0.0)]
SCENES = {
    # the floor meeting a vertical wall that runs away from the eye to the right: both in view from w = 1 to the horizon
    "crease": [FLOOR, [(np.array([0.1, 0.0, -1.0]) / np.hypot(0.1, 1.0), -0.5 / np.hypot(0.1, 1.0))]],  # z >= 0.5 + 0.1 x
    # a box on the floor, a vertical edge towards the eye: its faces are open, the floor at its foot is not
    "box_edge": [FLOOR, _box((2.6, 0.1), (0.9, BOX_TOP, 0.9), 0.6)],
}


@functools.lru_cache(maxsize=None)
def analytic_scene(name):
    """(depth f32 [h, w], normal f32 [h, w, 4], inv_viewproj, ppu, positions float64 [h, w, 3]) of SCENES[name]: every pixel
    centre's ray {M (xn, yn, z, 1)} cut with each face's plane in float64, the nearest cut inside its solid (reversed Z: the
    largest depth) taken, depth and normal rounded once.  A pixel that sees nothing holds depth 0 and a non-winner's normal."""
    w, h = SCENE
    inv_vp, ppu = camera(w, h, SCENE_CAMERA)
    M = matrix64(inv_vp)
    y, x = np.mgrid[0:h, 0:w]
    xn, yn = (x + 0.5) * 2.0 / w - 1.0, (y + 0.5) * 2.0 / h - 1.0
    A = M[:, 0] * xn[..., None] + M[:, 1] * yn[..., None] + M[:, 3]  # the ray's point at depth 0 ...
    B = M[:, 2]                                                     # ... and what a unit of depth adds
    best = np.zeros((h, w))
    positions, normal = np.zeros((h, w, 3)), np.zeros((h, w, 4))
    for solid in SCENES[name]:
        for n, d in solid:
            plane = np.array([*n, -d])
            with np.errstate(divide="ignore", invalid="ignore"):
                z = -(A @ plane) / (B @ plane)
                hh = A + z[..., None] * B
                X = hh[..., :3] / hh[..., 3:4]
                hit = (z > best) & (z <= 1.0)
                for n2, d2 in solid:
                    if n2 is not n:
                        hit &= X @ n2 <= d2
            best = np.where(hit, z, best)
            positions[hit] = X[hit]
            normal[hit] = (*n, 1.0)
    return best.astype(f32), normal.astype(f32), inv_vp, ppu, positions


@functools.lru_cache(maxsize=None)
def scene_statement(name):
    depth, normal, inv_vp, ppu, positions = analytic_scene(name)
    return ao64(depth, normal, inv_vp, ppu=ppu, positions=positions, **SCENE_PARAMS)


# ---------------------------------------------------------------- scissors and planes of the edge tests
# degenerate scissors, and scissors on the seams of the raw kernel's 32 x 32 tiles and 4-texel groups, over PLANE
EDGE_SCISSORS = {"1x1": (7, 9, 1, 1), "2x1": (8, 3, 2, 1), "1x5": (5, 4, 1, 5), "last_pixel": (129, 66, 1, 1),
                 "one_into_a_second_tile": (0, 0, 33, 33), "one_into_a_second_tile_at_the_end": (97, 34, 33, 33),
                 "narrower_than_a_group_31": (2, 1, 31, 32), "narrower_than_a_group_3": (6, 2, 3, 64)}


@functools.lru_cache(maxsize=None)
def small_plane(w, h=36):
    """(depth, normal, inv_viewproj, ppu) of a seeded random plane of a small extent"""
    inv_vp, ppu = camera(w, h)
    return (*random_gbuffer(w, h, seed=1000 + w), inv_vp, ppu)


def poisoned_outside(depth, normal, scissor, seed=5):
    """copies of the planes whose texels outside the scissor would show if they were read: depth a mix of NaN and near depths
    that would occlude (w of 0.11 to 0.4), normals NaN"""
    rng = np.random.default_rng(seed)
    inside = inside_of(depth.shape, scissor)
    bad = np.where(rng.random(depth.shape) < 0.5, np.nan, rng.uniform(0.25, 0.9, depth.shape)).astype(f32)
    return np.where(inside, depth, bad), np.where(inside[..., None], normal, f32(np.nan))


@functools.lru_cache(maxsize=None)
def special_plane():
    """(depth, normal, inv_viewproj, ppu) of a 68 x 36 random plane with the floats sprinkled in that a kernel could take
    another way than the contract: +inf, -0.0, negative and subnormal-positive depths; a normal w of -0.0 (non-zero bits: a
    winner), an infinite normal component, normals whose squared length underflows to a subnormal and to 0.  No NaN depth:
    include/svr_ambient.h leaves it unspecified."""
    depth, normal, inv_vp, ppu = small_plane(68)
    depth, normal = depth.copy(), normal.copy()
    rng = np.random.default_rng(11)
    zs = np.array([np.inf, -0.0, -0.25, 1e-41, 1.4e-45], f32)
    hit = rng.random(depth.shape) < 0.06
    depth[hit] = zs[rng.integers(0, zs.size, int(hit.sum()))]
    some = lambda share: rng.random(depth.shape) < share
    normal[some(0.03), 3] = f32(-0.0)
    ys, xs = np.nonzero(some(0.02))
    normal[ys, xs, rng.integers(0, 3, ys.size)] = f32(np.inf)
    normal[some(0.03), :3] = np.array([2e-20, -1e-20, 3e-21], f32)   # a squared length of about 5e-40: subnormal
    normal[some(0.03), :3] = np.array([1e-24, 2e-25, -1e-24], f32)   # ... of about 2e-48: 0 in fp32
    return depth, normal, inv_vp, ppu


def behind_the_eye(w, h):
    """(inv_viewproj, ppu): the camera's matrix with h.w = 0.5 xn added, so that the left of the plane has h.w < 0 wherever
    its clip w is above 2: surfaces behind the eye plane"""
    inv_vp, ppu = camera(w, h)
    inv_vp = inv_vp.copy()
    inv_vp[4 * 0 + 3] += f32(0.5)
    return inv_vp, ppu


def assert_behind_the_eye(ref, scissor):
    """the property of pixels with h.w < 0, on a reference's planes: each is "below one pixel" (raw (1, h.w), the 1/w negative
    as it came), and its blur accepted nothing but the centre although a darkened texel lay in its window"""
    m = inside_of(ref["out"].shape, scissor)
    neg = m & (ref["raw"][..., 1] < 0)
    assert neg[m].mean() > 0.05 and (ref["kind"][m] >= EVALUATED).any()
    assert (ref["kind"][neg] == SMALL).all() and (ref["raw"][..., 0][neg] == 1).all() and (ref["out"][neg] == 1).all()
    dark = m & (ref["raw"][..., 0] < 1)
    near = np.zeros_like(dark)
    h, w = dark.shape
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] |= dark[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    assert (neg & near).sum() >= 20, "a blur that accepted a neighbour would show"
