"""Test-side helpers of the temporal pass (include/svr_temporal.h): build and run tests/native/temporal_ref.cpp, the scalar
restatement of DESIGN C27-C31.  Colour and history images travel as uint16 [H, W, 4] arrays of fp16 bit patterns, as
Renderer.read_color gives them; depth as float32 [H, W]; reproject as a 4 x 4 indexed [col][row] like glmath's matrices."""
import functools

import numpy as np

import native_ref as N

f32 = np.float32
RESET, NO_CLAMP = 1, 2
WRONG_VARIANTS = {1: "min depth instead of max", 2: "no edge clamp at the scissor", 3: "hx without the -0.5", 4: "clamp after blend",
                  5: "fma(1, c - hc, hc) in place of c", 6: "vertical lerp before horizontal"}


ref_exe = functools.partial(N.build, "temporal_ref")


def identity():
    return np.eye(4, dtype=f32)


def run_ref(color, depth, history, reproject, blend, flags=0, history_valid=True, scissor=None, variant=0):
    """temporal_ref over one frame -> {"color": uint16 [H,W,4] after the pass, "history": the new history (zero outside
    the scissor), "valid": bool [H,W], the pixels that used the history}"""
    color = np.ascontiguousarray(color, dtype=np.uint16)
    h, w = color.shape[:2]
    assert color.shape == (h, w, 4)
    depth = np.ascontiguousarray(depth, dtype=f32)
    history = np.ascontiguousarray(history if history is not None else np.zeros_like(color), dtype=np.uint16)
    assert depth.shape == (h, w) and history.shape == (h, w, 4)
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    hdr = np.array([w, h, sx, sy, sw, sh, flags, 1 if history_valid and not flags & RESET else 0, variant], np.uint32).tobytes()
    par = np.concatenate([np.asarray(reproject, f32).reshape(16), np.array([blend], f32)]).astype(f32).tobytes()
    raw = N.run(ref_exe(), hdr + par + color.tobytes() + depth.tobytes() + history.tobytes())
    n = w * h
    assert len(raw) == n * 17
    return {"color": np.frombuffer(raw, np.uint16, n * 4, 0).reshape(h, w, 4).copy(),
            "history": np.frombuffer(raw, np.uint16, n * 4, n * 8).reshape(h, w, 4).copy(),
            "valid": np.frombuffer(raw, np.uint8, n, n * 16).reshape(h, w).astype(bool)}


def ndc_translation(dx_pixels, dy_pixels, w, h):
    """a reproject that moves every pixel's history position by whole pixels: NDC x += 2 dx / w (exact for powers of two)"""
    m = identity()
    m[3][0] = f32(2.0 * dx_pixels / w)
    m[3][1] = f32(2.0 * dy_pixels / h)
    return m


def random_depth(w, h, seed):
    """float32 [h, w] in [0, 1] with runs of exact 0 (cleared pixels: points at infinity)"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.0, 1.0, (h, w)).astype(f32)
    for _ in range(max(4, h // 4)):
        y, x, n = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(3, max(4, w // 2)))
        z[y, x:x + n] = 0.0
    return z
