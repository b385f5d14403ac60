"""Test-side helpers of the deferred lighting pass (include/svr_lighting.h): build and run tests/native/light_ref.cpp, the
scalar brute-force restatement of DESIGN C17-C19, and apply the stores of C20 to what it returns."""
import functools

import numpy as np

import __graft_entry__ as g
import native_ref as N

pkg = g.load_package()
A = pkg.abi
f32 = np.float32


ref_exe = functools.partial(N.build, "light_ref")


def m16(m):
    return np.ascontiguousarray(np.asarray(m, dtype=f32).reshape(16))


def inv_viewproj(viewproj16):
    """the inverse of a column-major float[16], computed in float64 (caller-computed: any rounding of it is an input)"""
    m = np.asarray(viewproj16, dtype=np.float64).reshape(4, 4).T
    return m16(np.linalg.inv(m).T)


def lighting_of(scene):
    return (np.array(scene.ambient_color, f32), np.array(scene.sunlight_direction, f32), np.array(scene.sunlight_color, f32))


def run_ref(depth, normal, albedo, inv_vp, ambient, sun_dir, sun_color, lights=None, shadow=None, shadow_vp=None, bias=0.0):
    """light_ref over whole planes -> {"rgba" f32 [H,W,4], "winner" bool [H,W], "position" f32 [H,W,3], "shadowed" bool [H,W]}"""
    h, w = depth.shape
    lights = np.zeros(0, A.POINT_LIGHT_DTYPE) if lights is None else np.ascontiguousarray(lights, dtype=A.POINT_LIGHT_DTYPE)
    hs, ws = shadow.shape if shadow is not None else (0, 0)
    parts = [np.array([w, h, lights.size, ws, hs], np.uint32).tobytes(), m16(inv_vp).tobytes()]
    parts += [np.asarray(v, f32).reshape(4).tobytes() for v in (ambient, sun_dir, sun_color)]
    parts += [m16(shadow_vp if shadow_vp is not None else np.zeros(16)).tobytes(), np.array([bias], f32).tobytes(), lights.tobytes()]
    parts += [np.ascontiguousarray(a, dtype=f32).tobytes() for a in (depth, normal, albedo)]
    if shadow is not None:
        parts.append(np.ascontiguousarray(shadow, dtype=f32).tobytes())
    raw = N.run(ref_exe(), b"".join(parts))
    n = w * h
    assert len(raw) == n * (16 + 1 + 12 + 1)
    return {"rgba": np.frombuffer(raw, f32, n * 4, 0).reshape(h, w, 4).copy(),
            "winner": np.frombuffer(raw, np.uint8, n, n * 16).reshape(h, w).astype(bool),
            "position": np.frombuffer(raw, f32, n * 3, n * 17).reshape(h, w, 3).copy(),
            "shadowed": np.frombuffer(raw, np.uint8, n, n * 29).reshape(h, w).astype(bool)}


def store(rgba, color_format):
    """C20: the colour target's texels of fp32 RGBA: fp16 bit patterns (RNE from float32), or unorm8 (clamp, * 255, RNE)"""
    rgba = np.asarray(rgba, dtype=f32)
    if color_format == A.COLOR_RGBA8:
        return np.rint(np.clip(rgba, f32(0), f32(1)) * f32(255)).astype(np.uint8)
    with np.errstate(over="ignore"):
        return rgba.astype(np.float16).view(np.uint16)


def expected_color(before, ref, color_format, owned=None):
    """the colour target after the pass: `before` with the reference's stored colour on the owned winner pixels"""
    out = before.copy()
    sel = ref["winner"] if owned is None else (ref["winner"] & owned)
    out[sel] = store(ref["rgba"], color_format)[sel]
    return out


def owned_mask(w, h, scissor=None, interleave=(1, 0)):
    x0, y0, sw, sh = scissor or (0, 0, w, h)
    m = np.zeros((h, w), bool)
    rows = np.arange(h)
    own = (rows >= y0) & (rows < y0 + sh) & ((((rows - y0) // 32) % interleave[0]) == interleave[1])
    m[own, x0:x0 + sw] = True
    return m
