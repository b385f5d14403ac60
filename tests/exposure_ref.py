"""Test-side helpers of auto-exposure (include/svr_exposure.h): build and run tests/native/exposure_ref.cpp, the scalar
restatement of DESIGN C38-C42, and an independent numpy fp64 statement of what the meter is for.  Colour targets travel as
uint16 [H, W, 4] arrays of fp16 bit patterns, as Renderer.read_color gives them; a state is a dict of SvrExposureState's
fields."""
import functools

import numpy as np

import native_ref as N
from native_ref import floats, halves  # noqa: F401  (re-exported)

f32 = np.float32
BINS = 256
FIRST_STATE = {"exposure": f32(1.0), "target": f32(1.0), "mean_log2": f32(0.0), "counted": 0, "black": 0, "meters": 0}
METER = {"key": 0.18, "low_fraction": 0.0, "high_fraction": 1.0, "min_exposure": 2.0 ** -10, "max_exposure": 2.0 ** 10, "adapt": 1.0}
WRONG_VARIANTS = {1: "bin shift off by one", 2: "black counted in bin 0", 3: "window over all pixels", 4: "floor for the window's upper end",
                  5: "clamp after the adapt step", 6: "snap ignored", 7: "sub-bin literals of the lower edges"}
STATE_DTYPE = np.dtype([("exposure", "<f4"), ("target", "<f4"), ("mean_log2", "<f4"), ("counted", "<u4"), ("black", "<u4"), ("meters", "<u4")])
ref_exe = functools.partial(N.build, "exposure_ref")


def meter(**kw):
    m = dict(METER)
    m.update(kw)
    return m


def state_of(st):
    """an abi.SvrExposureState (or a record of STATE_DTYPE) -> dict"""
    get = (lambda k: st[k]) if isinstance(st, np.void) else (lambda k: getattr(st, k))
    return {k: (f32(get(k)) if STATE_DTYPE[k].kind == "f" else int(get(k))) for k in STATE_DTYPE.names}


def state_bits(st):
    """the six words of a state, for bit-pattern comparisons"""
    a = np.zeros(1, STATE_DTYPE)
    for k in STATE_DTYPE.names:
        a[k] = st[k]
    return a.view(np.uint32).copy()


def run_ref(color, m=None, prev=None, snap=True, scissor=None, variant=0):
    """exposure_ref over a colour target -> (uint32 [256] histogram, the new state)"""
    color = np.ascontiguousarray(color, dtype=np.uint16)
    h, w = color.shape[:2]
    assert color.shape == (h, w, 4)
    m = m or METER
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, 1 if snap else 0, variant], np.uint32).tobytes()
    par = np.array([m["key"], m["low_fraction"], m["high_fraction"], m["min_exposure"], m["max_exposure"], m["adapt"]], f32).tobytes()
    raw = N.run(ref_exe(), hdr + par + state_bits(prev or FIRST_STATE).tobytes() + color.tobytes())
    assert len(raw) == BINS * 4 + 24
    return np.frombuffer(raw, np.uint32, BINS, 0).copy(), state_of(np.frombuffer(raw, STATE_DTYPE, 1, BINS * 4)[0])


def _floats_through(mode, values, out_dtype):
    values = np.ascontiguousarray(values, dtype=f32)
    return np.frombuffer(N.run(ref_exe(), values.tobytes(), mode), out_dtype).reshape(values.shape).copy()


def exp2_poly(x):
    """the contract's 2^x (C41) of a float32 array"""
    return _floats_through("--exp2", x, f32)


def counters(lum):
    """the counter (C39: 0 .. 255, 256 = black) of each luminance of a float32 array"""
    return _floats_through("--bin", lum, np.uint32)


def grey(h, w, value_bits, alpha=0x3c00):
    """a plane of one half in r, g and b"""
    out = np.empty((h, w, 4), np.uint16)
    out[..., :3] = value_bits
    out[..., 3] = alpha
    return out


def random_hdr(w, h, seed, specials=True, lo=-20.0, hi=16.0):
    """a seeded HDR colour target, uint16 [h, w, 4]: log2-uniform values from 2^lo up to 65504, a random alpha half and, with
    specials, texels of NaN, +-inf, negatives, -0, 65504, subnormal halves and exact bin edges 2^k (1 + j / 8) sprinkled in"""
    rng = np.random.default_rng(seed)
    v = np.minimum(2.0 ** rng.uniform(lo, hi, (h, w, 4)), 65504.0).astype(f32)
    out = halves(v)
    out[..., 3] = rng.integers(0, 1 << 16, (h, w), dtype=np.uint16)
    if specials:
        edges = halves([2.0 ** k * (1 + j / 8) for k in range(-14, 16) for j in range(8)])
        pool = np.concatenate([N.SPECIALS[:13], edges, edges - 1])
        hit = rng.random((h, w, 3)) < 0.04
        out[..., :3][hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
    return out


# ---------------------------------------------------------------- the independent fp64 statement
def luminance64(color, scissor=None):
    """the scissor's true luminances, fp64 [n]: san() per channel, Rec. 709 weights as decimal fp64 literals"""
    h, w = color.shape[:2]
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    with np.errstate(invalid="ignore"):
        c = floats(color[sy:sy + sh, sx:sx + sw, :3]).astype(np.float64).reshape(-1, 3)
        c = np.where(c > 0, np.minimum(c, 65504.0), 0.0)  # NaN compares false: 0
    return 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]


def statement64(color, m=None, scissor=None):
    """What the meter is for, without bins: of the pixels with luminance >= 2^-16, sorted, the ranks
    [floor(low T), ceil(high T)) are kept; -> (mean of np.log2 over the kept, key * 2.0 ** -mean clamped, T, kept), or
    (None, None, T, 0) for an empty window"""
    m = m or METER
    lum = np.sort(luminance64(color, scissor))
    lum = lum[lum >= 2.0 ** -16]
    T = lum.size
    lo, hi = int(np.floor(float(f32(m["low_fraction"])) * T)), int(np.ceil(float(f32(m["high_fraction"])) * T))
    kept = lum[lo:hi]
    if kept.size == 0:
        return None, None, T, 0
    mean = float(np.mean(np.log2(kept)))
    target = min(max(float(f32(m["key"])) * 2.0 ** -mean, float(f32(m["min_exposure"]))), float(f32(m["max_exposure"])))
    return mean, target, T, kept.size
