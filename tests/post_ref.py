"""Test-side helpers of the post pass (include/svr_post.h): build and run tests/native/post_ref.cpp, the scalar restatement
of DESIGN C22-C26.  Colour targets travel as uint16 [H, W, 4] arrays of fp16 bit patterns, as Renderer.read_color gives them."""
import functools

import numpy as np

import native_ref as N
from native_ref import floats, halves  # noqa: F401  (re-exported)

f32 = np.float32
CLAMP, REINHARD, ACES = 0, 1, 2
MAX_LEVELS = 8
WRONG_VARIANTS = {1: "edge clamp off by one", 2: "box on 2x-1", 3: "upsample weights swapped", 4: "threshold before the box",
                  5: "missing san", 6: "vertical before horizontal"}


ref_exe = functools.partial(N.build, "post_ref")


def level_extents(sw, sh, levels):
    """C22"""
    out, w, h = [], sw, sh
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def h16(values):
    """the reference's own fp32 -> fp16 rounding of a float32 array -> uint16 bit patterns"""
    values = np.ascontiguousarray(values, dtype=f32)
    return np.frombuffer(N.run(ref_exe(), values.tobytes(), "--h16"), np.uint16).reshape(values.shape).copy()


def roundtrip(bits):
    """h16(h2f()) of uint16 fp16 bit patterns, both the reference's own"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return np.frombuffer(N.run(ref_exe(), bits.tobytes(), "--roundtrip"), np.uint16).reshape(bits.shape).copy()


def run_ref(color, exposure=1.0, threshold=1.0, intensity=1.0, levels=4, tonemap=ACES, scissor=None, variant=0):
    """post_ref over a colour target -> {"color" uint16 [H,W,4] after the pass, "B" / "U": per level uint16 [h_i,w_i,4]}"""
    color = np.ascontiguousarray(color, dtype=np.uint16)
    h, w = color.shape[:2]
    assert color.shape == (h, w, 4)
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, levels, tonemap, variant], np.uint32).tobytes()
    par = np.array([exposure, threshold, intensity], f32).tobytes()
    raw = N.run(ref_exe(), hdr + par + color.tobytes())
    out = {"color": np.frombuffer(raw, np.uint16, w * h * 4, 0).reshape(h, w, 4).copy(), "B": [], "U": []}
    at = w * h * 8
    for lw, lh in level_extents(sw, sh, levels):
        assert tuple(np.frombuffer(raw, np.uint32, 2, at)) == (lw, lh)
        at += 8
        for key in ("B", "U"):
            out[key].append(np.frombuffer(raw, np.uint16, lw * lh * 4, at).reshape(lh, lw, 4).copy())
            at += lw * lh * 8
    assert at == len(raw)
    return out


def random_hdr(w, h, seed, specials=True, top=1.2, bright=200.0):
    """a seeded HDR colour target, uint16 [h, w, 4]: log-uniform values up to 10^top with spots `bright` times brighter, a random alpha half, and, with
    specials, texels of NaN, +-inf, negatives, -0, 65504 and subnormal halves sprinkled over it"""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-3, top, (h, w, 4))).astype(f32)
    spots = rng.random((h, w)) < 0.02
    v[spots] *= f32(bright)
    out = halves(v)
    out[..., 3] = rng.integers(0, 1 << 16, (h, w), dtype=np.uint16)
    if specials:
        pool = N.SPECIALS[:13]
        hit = rng.random((h, w, 3)) < 0.03
        out[..., :3][hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
    return out
