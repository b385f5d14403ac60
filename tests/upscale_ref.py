"""Test-side helpers of the upscaled present (include/svr_upscale.h): build and run tests/native/upscale_ref.cpp, the scalar
restatement of DESIGN C50-C54, and the inputs the tests share.  RGBA16F colour targets travel as uint16 [H, W, 4] arrays of
fp16 bit patterns, as Renderer.read_color gives them; RGBA8 ones as uint8 [H, W, 4]; destinations as uint8 [dh, dw, 4]."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import native_ref as N
from native_ref import floats, halves  # noqa: F401  (re-exported)

f32 = np.float32
BGRA, RGBA = 0, 1
NO_SHARPEN = 1
WRONG_VARIANTS = {1: "tap clamp off by one", 2: "w0 and w3 swapped", 3: "columns before rows", 4: "no anti-ringing clamp",
                  5: "sharpen reads quantised neighbours", 6: "sharpen's neighbours not clamped at the border"}
# source -> destination extents of the GPU tests (tests/test_upscale_gpu.py); the CPU tests use the small ones too
EXTENTS = [((1, 1), (5, 3)), ((2, 3), (70, 41)), ((37, 23), (61, 45)), ((16, 16), (64, 64)), ((33, 17), (33, 17)), ((40, 40), (40, 97)),
           ((96, 80), (160, 131)), ((7, 2), (16384, 2))]


ref_exe = functools.partial(N.build, "upscale_ref")


def run_ref(color, dw, dh, fmt=BGRA, sharpness=0.5, flags=0, variant=0, values=False):
    """upscale_ref over a colour target (uint16: RGBA16F, uint8: RGBA8) -> uint8 [dh, dw, 4], the destination's bytes; with
    values, (the bytes, float32 [dh, dw, 4]: what un8 was applied to, in R, G, B, A order)"""
    color = np.ascontiguousarray(color)
    assert color.dtype in (np.uint16, np.uint8) and color.ndim == 3 and color.shape[2] == 4
    h, w = color.shape[:2]
    hdr = np.array([w, h, dw, dh, 0 if color.dtype == np.uint16 else 1, fmt, flags, variant], np.uint32).tobytes()
    with tempfile.TemporaryDirectory(prefix="upscale_ref_io_") as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(hdr + np.array([sharpness], f32).tobytes() + color.tobytes())
        fval = os.path.join(d, "values.bin")
        subprocess.run([ref_exe(), fin, fout] + ([fval] if values else []), check=True)
        out = np.fromfile(fout, np.uint8).reshape(dh, dw, 4)
        return (out, np.fromfile(fval, f32).reshape(dh, dw, 4)) if values else out


def random_target(w, h, seed, specials=False):
    """a seeded RGBA16F colour target, uint16 [h, w, 4]: values on both sides of 0 and of 1 (about a sixth below 0 and a sixth
    above 1); with specials, NaN, +-inf, negative halves, -0 and subnormals sprinkled over it"""
    rng = np.random.default_rng(seed)
    out = halves(rng.uniform(-0.25, 1.25, (h, w, 4)))
    if specials:
        hit = rng.random((h, w, 4)) < 0.08
        out[hit] = N.SPECIALS[rng.integers(0, N.SPECIALS.size, int(hit.sum()))]
    return out


def checker(w, h, seed, cell=3, noise=0.04):
    """the hard-edged checker plus noise, uint16 [h, w, 4]: cells of `cell` texels alternating near 0.1 and near 0.9 (so the
    bicubic overshoots at every edge, and the edges reach the image border), each texel off by up to `noise`"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.where(((x // cell) + (y // cell)) % 2 == 0, 0.1, 0.9)[..., None]
    return halves(base + rng.uniform(-noise, noise, (h, w, 4)))


def finite_target(w, h, seed):
    """a seeded finite RGBA16F target in [0, 1), uint16 [h, w, 4]"""
    return halves(np.random.default_rng(seed).random((h, w, 4)))


def random_target8(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
