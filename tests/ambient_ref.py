"""Test-side helpers of the ambient pass (include/svr_ambient.h): build and run tests/native/ambient_ref.cpp, the scalar
restatement of DESIGN C32-C37 (and of C17-C19 with the ambient factor).  Depth travels as float32 [H, W], the normal plane
as float32 [H, W, 4], matrices as 4 x 4 indexed [col][row] like glmath's or as 16 floats, column-major."""
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


def run_ref(depth, normal, inv_vp, radius, ppu, bias=0.0, intensity=1.0, sharpness=0.05, flags=0, scissor=None):
    """ambient_ref ao over one frame -> {"raw": f32 [H,W,2], "out": f32 [H,W], "kind": uint8 [H,W]}; zeros outside the scissor"""
    depth = np.ascontiguousarray(depth, dtype=f32)
    h, w = depth.shape
    normal = np.ascontiguousarray(normal, dtype=f32)
    assert normal.shape == (h, w, 4)
    sx, sy, sw, sh = scissor or (0, 0, w, h)
    blob = np.array([w, h, sx, sy, sw, sh, flags], np.uint32).tobytes() + m16(inv_vp).tobytes() + \
        np.array([radius, ppu, bias, intensity, sharpness], f32).tobytes() + depth.tobytes() + normal.tobytes()
    n = w * h
    raw = _run("ao", blob, n * 13)
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
