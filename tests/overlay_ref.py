"""Test-side helpers of the UI overlay pass (include/svr_overlay.h): build and run tests/native/overlay_ref.cpp, the
scalar restatement of DESIGN C43-C49, and make the lists the tests draw.  A list is a dict: vertices
(abi.OVERLAY_VERTEX_DTYPE), indices (uint16), cmds (abi.OVERLAY_CMD_DTYPE), textures (a list of (texels, width, height,
format), texels a uint8 array [h, w, 4] or [h, w]), display_pos and scale.  Images are uint32 [H, W] arrays of texel words."""
import functools

import numpy as np

import __graft_entry__ as g
import native_ref as N

A = g.load_package().abi
f32 = np.float32
BGRA, RGBA = 0, 1  # SVR_SWAPCHAIN_*
WRONG_VARIANTS = {1: "the top-left rule mirrored", 2: "centres at corners", 3: "no quantisation between layers", 4: "reversed order",
                  5: "clip rounded instead of truncated", 6: "R/B swapped for the wrong format", 7: "A8 read as grey",
                  8: "wrap instead of clamp", 9: "premultiplied blend"}
NO_CLIP = (-1.0e6, -1.0e6, 1.0e6, 1.0e6)
ref_exe = functools.partial(N.build, "overlay_ref")


def pack(r, g_, b, a=255):
    return (int(r) & 255) | ((int(g_) & 255) << 8) | ((int(b) & 255) << 16) | ((int(a) & 255) << 24)


def white_texture():
    """a 1 x 1 opaque white RGBA8 texture"""
    return (np.full((1, 1, 4), 255, np.uint8), 1, 1, A.OVERLAY_TEX_RGBA8)


def make_list(vertices, indices=None, cmds=None, textures=None, display_pos=(0.0, 0.0), scale=(1.0, 1.0)):
    """vertices: records, or rows (x, y, u, v, col).  Without indices: 0, 1, 2, ...; without cmds: one unclipped command over
    everything with texture 0; without textures: one opaque white texel"""
    if not (isinstance(vertices, np.ndarray) and vertices.dtype == A.OVERLAY_VERTEX_DTYPE):
        rows = list(vertices)
        vertices = np.zeros(len(rows), A.OVERLAY_VERTEX_DTYPE)
        for k, (x, y, u, v, col) in enumerate(rows):
            vertices[k] = ((x, y), (u, v), col)
    indices = np.arange(len(vertices), dtype=np.uint16) if indices is None else np.asarray(indices, dtype=np.uint16)
    if cmds is None:
        cmds = [(NO_CLIP, 0, 0, 0, len(indices))]
    if not (isinstance(cmds, np.ndarray) and cmds.dtype == A.OVERLAY_CMD_DTYPE):
        rows = list(cmds)
        cmds = np.zeros(len(rows), A.OVERLAY_CMD_DTYPE)
        for k, row in enumerate(rows):
            cmds[k] = tuple(row)
    return {"vertices": vertices, "indices": indices, "cmds": cmds, "textures": [white_texture()] if textures is None else list(textures),
            "display_pos": tuple(display_pos), "scale": tuple(scale)}


def tri(p0, p1, p2, col=0xffffffff, uv=((0.5, 0.5),) * 3):
    """three vertex rows"""
    cols = col if isinstance(col, (tuple, list)) else (col,) * 3
    return [(p[0], p[1], t[0], t[1], c) for p, t, c in zip((p0, p1, p2), uv, cols)]


def run_ref(image, fmt, lst, variant=0):
    """overlay_ref over an image -> (the image after, uint32 [H, W] fragments per pixel, {triangles, kept, tiles})"""
    image = np.ascontiguousarray(image, dtype=np.uint32)
    h, w = image.shape
    idx = lst["indices"]
    if idx.size % 2:
        idx = np.concatenate([idx, np.zeros(1, np.uint16)])
    parts = [np.array([w, h, fmt, variant, lst["vertices"].size, lst["indices"].size, lst["cmds"].size, len(lst["textures"])], np.uint32).tobytes(),
             np.array(list(lst["display_pos"]) + list(lst["scale"]), f32).tobytes(), lst["vertices"].tobytes(), idx.tobytes(), lst["cmds"].tobytes()]
    for texels, tw, th, tf in lst["textures"]:
        raw = np.ascontiguousarray(texels, dtype=np.uint8).tobytes()
        assert len(raw) == tw * th * (1 if tf == A.OVERLAY_TEX_A8 else 4)
        parts += [np.array([tw, th, tf, 0], np.uint32).tobytes(), raw + b"\0" * (-len(raw) % 4)]
    parts.append(image.tobytes())
    raw = np.frombuffer(N.run(ref_exe(), b"".join(parts)), np.uint32)
    assert raw.size == 2 * w * h + 3
    stats = dict(zip(("triangles", "kept", "tiles"), (int(v) for v in raw[2 * w * h:])))
    return raw[:w * h].reshape(h, w).copy(), raw[w * h:2 * w * h].reshape(h, w).copy(), stats


def random_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)


def random_texture(w, h, fmt, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if fmt == A.OVERLAY_TEX_A8 else (h, w, 4)
    return (rng.integers(0, 256, shape, dtype=np.uint8), w, h, fmt)


def soup(n, w, h, seed, n_textures=1):
    """n seeded random triangles around a w x h image: random colours and alpha per vertex, both windings, degenerate ones,
    vertices off screen and some beyond the +-2^15 px clamp, uv in and beyond [0, 1]"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        kind = rng.integers(0, 10)
        centre = rng.uniform((-8, -8), (w + 8, h + 8))
        size = rng.choice([1.5, 6.0, 20.0, 60.0])
        p = centre + rng.uniform(-size, size, (3, 2))
        if kind == 0:
            p[2] = p[1]  # zero area
        elif kind == 1:
            p[2] = p[0] + 2.0 * (p[1] - p[0])  # collinear (up to rounding)
        elif kind == 2:
            p[rng.integers(0, 3)] = rng.choice([-1.0, 1.0], 2) * rng.uniform(3.0e4, 9.0e4, 2)  # beyond the snap's clamp
        elif kind == 3:
            p = np.round(p * 2.0) / 2.0  # vertices on pixel centres and corners
        cols = [pack(*rng.integers(0, 256, 4)) for _ in range(3)]
        uvs = rng.uniform(-0.3, 1.3, (3, 2))
        rows += [(f32(p[i][0]), f32(p[i][1]), f32(uvs[i][0]), f32(uvs[i][1]), cols[i]) for i in range(3)]
    return rows
