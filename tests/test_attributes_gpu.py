"""Attribute targets (include/svr_attributes.h) on the MI355X.

The CPU oracle has no attribute planes, but its per-pixel trace (svr_debug_trace_pixel) fills the same slots the planes
hold: with the transparent list empty, the last fragment-shader invocation it keeps at a pixel is the opaque winner's.
So the expected texel of every checked pixel is one traced oracle pass.  Besides that every path that builds draw
records and every tile-kernel variant must give the same planes, enabling them must change nothing else, and they must
agree with the ID target.  Every comparison is on bit patterns, with no tolerance."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T
from test_ids_gpu import HIP_STATS, ISOLATED, TUNE_HIZ, TUNE_NO_HIZ, TUNE_NO_SPLIT, _objects, assert_frames_same, assert_ids_same

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu

ATTRS = (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)
EVERY_PIXEL_MAX = 8192  # frames of up to this many pixels are checked at every pixel ...
SAMPLES, MIN_WINNERS = 4096, 1024  # ... larger ones at this many seeded pixels, of which this many must have a winner
# larger frames that are checked at every pixel all the same: "fan" (96x96) has no opaque object, so no sample of it could
# hold MIN_WINNERS winners; all of its 9216 pixels must be all-zero texels
EVERY_PIXEL = {"fan"}
PATTERN = 0x7FC5A5A5  # what untouched texels hold (a NaN: compared as bits)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_planes_same(a, b, what, where=None):
    for attr in ATTRS:
        if attr not in a and attr not in b:
            continue
        x, y = bits(a[attr]), bits(b[attr])
        bad = np.any(x != y, axis=-1)
        if where is not None:
            bad &= where
        assert not bad.any(), f"{what}: attribute {attr}: {int(bad.sum())} texels differ, first at (y, x) = {np.argwhere(bad)[0].tolist()}"


def read_planes(r, mask=A.ATTR_ALL):
    return {attr: r.read_attribute(attr) for attr in ATTRS if mask & attr}


def expected_texels(trace):
    """the four texels of a pixel from the oracle's trace of it (slot 0 == 0: no opaque fragment)"""
    t = np.asarray(trace, dtype=np.float32)
    if t[0] == 0.0:
        return {A.ATTR_BARY: np.zeros(4, np.float32), A.ATTR_UV: np.zeros(2, np.float32),
                A.ATTR_NORMAL: np.zeros(4, np.float32), A.ATTR_ALBEDO: np.zeros(4, np.float32)}
    return {A.ATTR_BARY: np.array([t[1], t[2], t[3], 0.0], np.float32), A.ATTR_UV: np.array([t[4], t[5]], np.float32),
            A.ATTR_NORMAL: np.array([t[15], t[16], t[17], t[21]], np.float32),
            A.ATTR_ALBEDO: np.array([t[18], t[19], t[20], 1.0], np.float32)}


def pixels_to_check(w, h, seed=2024, every=False):
    if every or w * h <= EVERY_PIXEL_MAX:
        return [(x, y) for y in range(h) for x in range(w)]
    rng = np.random.default_rng(seed)
    flat = rng.choice(w * h, SAMPLES, replace=False)
    return [(int(i % w), int(i // w)) for i in flat]


def oracle_traces(r, scene, opaque, pixels, draw=None):
    """one traced opaque-only pass of the oracle per pixel, in one context"""
    draw = draw or A.Renderer.draw_geometry
    empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
    out = []
    for x, y in pixels:
        r.trace_pixel(x, y)
        draw(r, scene, opaque, empty)
        out.append(r.read_trace().copy())
    return out


def assert_planes_match_traces(planes, pixels, traces, what, min_winners=0):
    winners = 0
    for (x, y), t in zip(pixels, traces):
        want = expected_texels(t)
        winners += int(t[0] != 0.0)
        for attr in ATTRS:
            got = planes[attr][y, x]
            assert np.array_equal(bits(got), bits(want[attr])), \
                f"{what}: pixel ({x}, {y}) attribute {attr}: {got.tolist()} (bits {bits(got).tolist()}), the oracle's trace gives {want[attr].tolist()} (bits {bits(want[attr]).tolist()})"
    assert winners >= min_winners, f"{what}: only {winners} checked pixels have an opaque winner"
    return winners


def run(lib, name, mp, attrs=A.ATTR_ALL, ids=False, path="host", options=(), trace=False, bound=False, every_pixel=False):
    """Scenario `name` with its draw_geometry call rerouted.  HIP library: attribute planes of `attrs` (0: none; bound:
    pattern-filled torch tensors instead of the context's zeroed planes), an ID target or not, the host flatten, the device
    flatten or a draw list, extra options; the frame of T._finish plus "attr" {bit: plane} and "ids".  Oracle
    (trace=True): a traced opaque-only pass per checked pixel before the frame's own; the frame plus "pixels" and
    "traces"."""
    orig_draw, orig_finish = A.Renderer.draw_geometry, T._finish
    extra = {}

    def draw(self, scene, opaque, transparent=None):
        op, tr = _objects(opaque), _objects(transparent)
        if trace:
            extra["pixels"] = pixels_to_check(self.width, self.height, every=every_pixel)
            extra["traces"] = oracle_traces(self, scene, op, extra["pixels"], orig_draw)
            return orig_draw(self, scene, op, tr)
        for k, v in options:
            self.set_option(k, v)
        if attrs and bound:
            _torch, extra["tensors"] = _torch_planes(self.width, self.height)
            for attr in ATTRS:
                if attrs & attr:
                    self.bind_attribute_target(attr, extra["tensors"][attr].data_ptr())
        elif attrs:
            self.enable_attributes(attrs)
        if ids:
            self.enable_ids()
        self.set_option(A.OPT_DEVICE_FLATTEN, 1 if path == "device" else 2)
        if path == "list":
            lst = self.create_draw_list(op, tr)
            st = self.draw_list(scene, lst)
            lst.close()
            return st
        return orig_draw(self, scene, op, tr)

    def finish(r, stats=None):
        out = orig_finish(r, stats)
        if not trace:
            out["attr"] = read_planes(r, attrs)
            if ids:
                out["ids"] = r.read_ids()
        out.update({k: v for k, v in extra.items() if k != "tensors"})
        return out

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        m.setattr(T, "_finish", finish)
        return SC.SCENARIOS[name](lib)


def assert_planes_agree_with_ids(planes, ids, what):
    """r of the BARY plane is nonzero exactly where the ID target names an object; every plane is zero elsewhere"""
    won = ids[..., 0] != 0
    assert np.array_equal(bits(planes[A.ATTR_BARY])[..., 2] != 0, won), what
    for attr in ATTRS:
        assert not bits(planes[attr])[~won].any(), f"{what}: attribute {attr} is not zero where no opaque fragment won"
    assert np.all(bits(planes[A.ATTR_ALBEDO])[..., 3][won] == 0x3F800000), what
    assert not bits(planes[A.ATTR_BARY])[..., 3].any(), what


# ---------------------------------------------------------------- 1. against the oracle, pixel by pixel
@pytest.mark.parametrize("name", ISOLATED + ["hiz_depth_extremes"])
def test_planes_against_the_oracle_trace(hip, oracle, name, monkeypatch):
    got = run(hip, name, monkeypatch)
    want = run(oracle, name, monkeypatch, trace=True, every_pixel=name in EVERY_PIXEL)
    T.assert_images_identical(got["depth"], want["depth"], name + " depth")
    h, w = got["depth"].shape
    n = len(want["pixels"])
    sampled = w * h > EVERY_PIXEL_MAX and name not in EVERY_PIXEL
    assert n == (SAMPLES if sampled else w * h)
    # a sampled frame must have an opaque winner at MIN_WINNERS of its checked pixels
    winners = assert_planes_match_traces(got["attr"], want["pixels"], want["traces"], name, min_winners=MIN_WINNERS if sampled else 0)
    print(f"{name}: {w}x{h}, {n} pixels checked, {winners} with an opaque winner")


def _atrium(lib, w, h, color_format=0, lod=8, tex_size=64):
    return T.setup_sponza(lib, w, h, lod=lod, tex_size=tex_size, color_format=color_format)


@pytest.mark.parametrize("size", [(96, 64), (150, 100)])
def test_atrium_against_the_oracle_trace(hip, oracle, size):
    w, h = size
    r, scene, opaque, transparent = _atrium(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    planes, depth = read_planes(r), r.read_depth()
    r.close()
    o, scene, opaque, transparent = _atrium(oracle, w, h)
    o.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    pixels = pixels_to_check(w, h)
    traces = oracle_traces(o, scene, opaque, pixels)
    o.draw_geometry(scene, opaque, transparent)
    T.assert_images_identical(depth, o.read_depth(), f"atrium {w}x{h} depth")
    o.close()
    every = w * h <= EVERY_PIXEL_MAX
    assert len(pixels) == (w * h if every else SAMPLES)
    winners = assert_planes_match_traces(planes, pixels, traces, f"atrium {w}x{h}", min_winners=len(pixels) if (w, h) == (96, 64) else MIN_WINNERS)
    print(f"atrium {w}x{h}: {len(pixels)} pixels checked, {winners} with an opaque winner")


# ---------------------------------------------------------------- 2. every path gives the same planes
VARIANT_SCENARIOS = ["soup", "soup_rgba8", "soup_scissor", "soup_odd_size", "soup_dense_split", "near_clip_wall", "floor_trilinear",
                     "transparent_stack_230", "hiz_depth_extremes", "ragged"]


@pytest.mark.parametrize("name", VARIANT_SCENARIOS)
def test_every_path_and_variant_gives_the_same_planes(hip, name, monkeypatch):
    first = run(hip, name, monkeypatch, ids=True)
    assert_planes_agree_with_ids(first["attr"], first["ids"], name)
    for path in ("device", "list"):
        got = run(hip, name, monkeypatch, path=path)
        assert_planes_same(got["attr"], first["attr"], f"{name} {path}")
    for opts in (((A.OPT_COUNT_FRAGMENTS, 0),), ((A.OPT_TUNING, TUNE_NO_HIZ),), ((A.OPT_TUNING, TUNE_HIZ),),
                 ((A.OPT_COUNT_FRAGMENTS, 0), (A.OPT_TUNING, TUNE_HIZ)), ((A.OPT_COUNT_FRAGMENTS, 0), (A.OPT_TUNING, TUNE_NO_HIZ)),
                 ((A.OPT_TUNING, TUNE_NO_SPLIT),), ((A.OPT_COUNT_FRAGMENTS, 0), (A.OPT_TUNING, TUNE_NO_SPLIT))):
        got = run(hip, name, monkeypatch, options=opts)
        assert_planes_same(got["attr"], first["attr"], f"{name} {opts}")
    for attr in ATTRS:  # a single plane against the same plane of all four
        got = run(hip, name, monkeypatch, attrs=attr, options=((A.OPT_COUNT_FRAGMENTS, 0),))
        assert set(got["attr"]) == {attr}
        assert_planes_same(got["attr"], {attr: first["attr"][attr]}, f"{name} plane {attr} alone")


def _atrium_planes(hip, w=256, h=144, color_format=0, options=(), path="host", prepare=None, mask=A.ATTR_ALL):
    r, scene, opaque, transparent = _atrium(hip, w, h, color_format)
    for k, v in options:
        r.set_option(k, v)
    r.enable_attributes(mask)
    if prepare:
        prepare(r, scene, opaque, transparent)
    r.clear_color((1, 1, 1, 1))
    if path == "list":
        lst = r.create_draw_list(opaque, transparent)
        r.draw_list(scene, lst)
        lst.close()
    else:
        r.set_option(A.OPT_DEVICE_FLATTEN, 1 if path == "device" else 2)
        r.draw_geometry(scene, opaque, transparent)
    out = {"attr": read_planes(r, mask), "color": r.read_color(), "depth": r.read_depth(), "stats": r.get_stats()}
    r.close()
    return out


def test_atrium_paths_formats_replay_and_occlusion(hip):
    base = _atrium_planes(hip)
    assert bits(base["attr"][A.ATTR_BARY])[..., 2].all()  # the atrium covers the frame
    for path in ("device", "list"):
        assert_planes_same(_atrium_planes(hip, path=path)["attr"], base["attr"], path)
    for opts in (((A.OPT_COUNT_FRAGMENTS, 1),), ((A.OPT_TUNING, TUNE_NO_HIZ),), ((A.OPT_TUNING, TUNE_HIZ),)):
        assert_planes_same(_atrium_planes(hip, options=opts)["attr"], base["attr"], str(opts))
    assert_planes_same(_atrium_planes(hip, color_format=A.COLOR_RGBA8)["attr"], base["attr"], "rgba8")
    # a tiny queue capacity: the pass overflows, writes nothing, and is replayed
    got = _atrium_planes(hip, options=((A.OPT_QUEUE_CAPS, 64),))
    assert got["stats"].replayed_passes > 0
    assert_planes_same(got["attr"], base["attr"], "replayed")
    T.assert_images_identical(got["color"], base["color"], "replayed colour")

    # an occlusion pyramid built from a depth-only prepass of a subset of the objects: the winners are the same
    def occlusion(r, scene, opaque, transparent):
        pyr = r.create_depth_pyramid()
        r.draw_depth(scene, opaque[::3])
        r.build_depth_pyramid(pyr)
        r.set_occlusion_pyramid(pyr)
    for path in ("host", "list"):
        got = _atrium_planes(hip, prepare=occlusion, path=path)
        assert_planes_same(got["attr"], base["attr"], f"occlusion {path}")
        T.assert_images_identical(got["depth"], base["depth"], "occlusion depth")


def _torch_planes(w, h):
    torch = pytest.importorskip("torch")
    t = {attr: torch.full((h, w, A.ATTR_FLOATS[attr]), PATTERN, dtype=torch.int32, device="cuda") for attr in ATTRS}
    torch.cuda.synchronize()
    return torch, t


def _tensor_bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_scissor_interleave_and_caller_bound_planes(hip):
    w, h = 256, 144
    r, scene, opaque, transparent = _atrium(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.draw_geometry(scene, opaque, transparent)
    full = read_planes(r)
    torch, t = _torch_planes(w, h)
    for attr in ATTRS:
        r.bind_attribute_target(attr, t[attr].data_ptr())
        assert r.get_attribute_target(attr) == t[attr].data_ptr()
    r.draw_geometry(scene, opaque, transparent)
    r.sync()
    for attr in ATTRS:  # caller-bound planes against context-owned ones
        assert np.array_equal(_tensor_bits(t[attr]), bits(full[attr])), attr
    for attr in ATTRS:
        t[attr].fill_(PATTERN)
    torch.cuda.synchronize()
    x0, y0, sw, sh = 37, 21, 101, 77
    r.set_scissor(x0, y0, sw, sh)
    r.draw_geometry(scene, opaque, transparent)
    got = read_planes(r)
    mask = np.zeros((h, w), bool)
    mask[y0:y0 + sh, x0:x0 + sw] = True
    for attr in ATTRS:
        assert np.array_equal(bits(got[attr])[mask], bits(full[attr])[mask]), f"scissor {attr}"
        assert np.all(bits(got[attr])[~mask] == PATTERN), f"scissor {attr}: texels outside it were written"
        assert np.array_equal(_tensor_bits(t[attr]), bits(got[attr]))
    # interleaved rows: of the 32-row tile rows, those with index % 3 == 1
    for attr in ATTRS:
        t[attr].fill_(PATTERN)
    torch.cuda.synchronize()
    r.set_scissor(0, 0, w, h)
    r.set_row_interleave(3, 1)
    r.draw_geometry(scene, opaque, transparent)
    got = read_planes(r)
    rows = (np.arange(h) // 32) % 3 == 1
    for attr in ATTRS:
        assert np.array_equal(bits(got[attr])[rows], bits(full[attr])[rows]), f"interleave {attr}"
        assert np.all(bits(got[attr])[~rows] == PATTERN), f"interleave {attr}: rows of other ranks were written"
    r.set_row_interleave(1, 0)
    for attr in ATTRS:
        r.bind_attribute_target(attr, None)
    assert_planes_same(read_planes(r), full, "back to the context's planes")
    r.close()


# scenarios with pixels no opaque fragment wins, none of them under a scissor (soup_scissor has a winner at every pixel of
# its scissor; what a scissor leaves alone is test_scissor_interleave_and_caller_bound_planes' matter)
@pytest.mark.parametrize("name", ["depth_later_nearer", "soup_opaque_only", "soup_odd_size", "ragged", "empty"])
def test_pixels_without_a_winner_are_cleared(hip, name, monkeypatch):
    """'cleared and written': a pixel the pass owns and no opaque fragment won becomes all zero, whatever the plane held"""
    want = run(hip, name, monkeypatch)  # the context's planes, zeroed when they were made
    got = run(hip, name, monkeypatch, bound=True)  # planes full of PATTERN
    h, w = got["depth"].shape
    empty = bits(want["attr"][A.ATTR_BARY])[..., 2] == 0
    assert empty.sum() >= 64, f"{name}: the scenario has too few pixels without a winner to show anything"
    for attr in ATTRS:
        g_, w_ = bits(got["attr"][attr]), bits(want["attr"][attr])
        assert not g_[empty].any(), f"{name}: attribute {attr} keeps old data where no opaque fragment won"
        assert np.array_equal(g_, w_), f"{name}: attribute {attr}"


def test_odd_origin_scissor_against_the_oracle_trace(hip, oracle):
    """Large textured triangles under a scissor with an odd origin: fully covered 8x8 blocks whose lanes are not quad
    partners.  The attribute pass follows the contract there: planes equal the oracle's trace and colour the oracle's."""
    w, h = 256, 144
    x0, y0, sw, sh = 37, 21, 101, 77
    r, scene, opaque, transparent = _atrium(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.clear_color((1, 1, 1, 1))
    r.set_scissor(x0, y0, sw, sh)
    r.draw_geometry(scene, opaque, transparent)
    planes, color, depth = read_planes(r), r.read_color(), r.read_depth()
    r.close()
    o, scene, opaque, transparent = _atrium(oracle, w, h)
    o.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    o.clear_color((1, 1, 1, 1))
    o.set_scissor(x0, y0, sw, sh)
    o.draw_geometry(scene, opaque, transparent)
    T.assert_images_identical(depth, o.read_depth(), "odd-origin scissor depth")
    T.assert_images_identical(color[y0:y0 + sh, x0:x0 + sw], o.read_color()[y0:y0 + sh, x0:x0 + sw], "odd-origin scissor colour")
    rng = np.random.default_rng(2024)
    inside = [(x0 + int(i % sw), y0 + int(i // sw)) for i in rng.choice(sw * sh, SAMPLES, replace=False)]
    outside = [(x0 - 1, y0), (x0, y0 - 1), (x0 + sw, y0 + sh - 1), (x0 + sw - 1, y0 + sh), (0, 0), (w - 1, h - 1)]
    traces = oracle_traces(o, scene, opaque, inside + outside)
    o.close()
    winners = assert_planes_match_traces(planes, inside + outside, traces, "odd-origin scissor", min_winners=MIN_WINNERS)
    assert winners == len(inside)  # the atrium covers the frame; outside the scissor nothing is traced or written
    print(f"odd-origin scissor: {len(inside) + len(outside)} pixels checked, {winners} with an opaque winner")


def test_other_passes_leave_the_planes_untouched(hip):
    w, h = 128, 96
    r, scene, opaque, transparent = _atrium(hip, w, h)
    torch, t = _torch_planes(w, h)
    for attr in ATTRS:
        r.bind_attribute_target(attr, t[attr].data_ptr())
    r.clear_color((0.5, 0.5, 0.5, 1))
    r.draw_background(0, A.GRADIENT_DEFAULT)
    r.draw_colored_triangle()
    cube = S.cube_mesh()
    mesh = r.upload_mesh(cube.indices, cube.vertices)
    img = r.create_image(S.checkerboard_32(), mipmapped=False)
    smp = r.create_sampler(**S.SAMPLER_NEAREST)
    r.draw_tex_image(mesh, 0, cube.indices.size, S.config2_render_matrix(w, h), img, smp)
    r.draw_depth(scene, opaque)  # a depth-only pass
    fmt_words = 2  # RGBA16F
    color = torch.zeros((2, h, w, fmt_words), dtype=torch.int32, device="cuda")
    depth = torch.zeros((2, h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.draw_views([scene, scene], color.data_ptr(), depth.data_ptr(), opaque, transparent, clear_rgba=(1, 1, 1, 1))  # a multiview pass
    r.sync()
    assert depth.cpu().numpy().any()
    for attr in ATTRS:
        assert np.all(_tensor_bits(t[attr]) == PATTERN), f"attribute {attr} was written by a pass that is not a geometry pass"
    r.draw_geometry(scene, opaque, transparent)  # ... and the geometry pass does write them
    r.sync()
    for attr in ATTRS:
        assert not np.any(_tensor_bits(t[attr]) == PATTERN), attr
    r.close()


def test_replay_writes_the_planes_of_its_pass(hip):
    w, h = 256, 144
    want = _atrium_planes(hip, w, h)["attr"]
    r, scene, opaque, transparent = _atrium(hip, w, h)
    r.set_option(A.OPT_QUEUE_CAPS, 64)
    r.set_option(A.OPT_TUNING, 16)  # TUNE_NO_POLL: the overflow is found at the fence, after the unbind below
    torch, t = _torch_planes(w, h)
    for attr in ATTRS:
        r.bind_attribute_target(attr, t[attr].data_ptr())
    r.draw_geometry(scene, opaque, transparent)
    for attr in ATTRS:
        r.bind_attribute_target(attr, None)  # no planes from here on: the pass and its replay still write t
    r.sync()
    assert r.get_stats().replayed_passes > 0
    for attr in ATTRS:
        assert r.get_attribute_target(attr) is None
        assert np.array_equal(_tensor_bits(t[attr]), bits(want[attr])), f"replayed pass, attribute {attr}"
        with pytest.raises(A.SvrError, match="no such plane"):
            r.read_attribute(attr)
    r.close()


def test_errors_are_refused(hip):
    r = hip.create(64, 32)
    L = hip.lib
    for bad in (0, 3, 16, A.ATTR_ALL):
        with pytest.raises(A.SvrError):
            r.bind_attribute_target(bad, None)
        with pytest.raises(A.SvrError):
            r.get_attribute_target(bad)
    with pytest.raises(A.SvrError):
        r.enable_attributes(16)
    with pytest.raises(A.SvrError, match="no such plane"):
        r.read_attribute(A.ATTR_UV)
    r.enable_attributes(A.ATTR_UV | A.ATTR_NORMAL)
    assert r.get_attribute_target(A.ATTR_BARY) is None and r.get_attribute_target(A.ATTR_UV)
    assert r.read_attribute(A.ATTR_UV).shape == (32, 64, 2) and not r.read_attribute(A.ATTR_NORMAL).any()
    buf = np.zeros(64 * 32 * 4, np.float32)
    assert L.svr_read_attribute(r.h, A.ATTR_UV, buf.ctypes.data, buf.nbytes) == -1  # the NORMAL plane's size, not the UV plane's
    assert L.svr_bind_attribute_target(r.h, A.ATTR_UV, 8) == -1  # misaligned
    r.enable_attributes(A.ATTR_NORMAL)  # UV's bit cleared: its plane is freed
    assert r.get_attribute_target(A.ATTR_UV) is None
    r.close()


# ---------------------------------------------------------------- 3. nothing else changes; 4. consistency with the IDs
@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_planes_change_nothing_else(hip, name, monkeypatch):
    want = run(hip, name, monkeypatch, attrs=0, ids=True)
    got = run(hip, name, monkeypatch, ids=True)
    assert_frames_same(got, want, name)
    assert_ids_same(got["ids"], want["ids"], name)
    assert_planes_agree_with_ids(got["attr"], got["ids"], name)
    plain = run(hip, name, monkeypatch, attrs=0)
    no_ids = run(hip, name, monkeypatch)  # planes without an ID target
    assert_frames_same(no_ids, plain, name + " without IDs")
    assert_planes_same(no_ids["attr"], got["attr"], name + " without IDs")


def test_disabling_the_planes_brings_the_old_pass_back(hip):
    w, h = 256, 144
    want = {}
    r, scene, opaque, transparent = _atrium(hip, w, h)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    want = T._finish(r)
    r.enable_attributes(A.ATTR_ALL)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    assert_frames_same(T._finish(r), want, "with planes")
    r.enable_attributes(0)
    for attr in ATTRS:
        assert r.get_attribute_target(attr) is None
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    assert_frames_same(T._finish(r), want, "after svr_enable_attributes(0)")
    with pytest.raises(A.SvrError, match="no such plane"):
        r.read_attribute(A.ATTR_BARY)
    r.close()


# ---------------------------------------------------------------- 5. full size once
def test_full_size_frame_with_all_four_planes(hip, oracle):
    import test_full_frames as FF
    MF = FF.MF
    name = "config3_3840x2160"
    w, h, _ = MF.FRAMES[name]
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=MF.TEX)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    color, depth, ids, planes = r.read_color(), r.read_depth(), r.read_ids(), read_planes(r)
    r.close()
    with open(MF.OUT) as f:
        d = json.load(f)[name]
    assert MF.sha(color) == d["color"] and MF.sha(depth) == d["depth"]
    assert_planes_agree_with_ids(planes, ids, name)
    ys, xs = np.nonzero(ids[..., 0])
    rng = np.random.default_rng(64)
    pick = rng.choice(len(ys), 64, replace=False)
    pixels = [(int(xs[i]), int(ys[i])) for i in pick]
    o, scene, opaque, transparent = T.setup_sponza(oracle, w, h, lod=1, tex_size=MF.TEX)
    oracle.lib.svr_oracle_set_threads(o.h, min(16, len(os.sched_getaffinity(0))))
    o.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    traces = oracle_traces(o, scene, opaque, pixels)
    o.close()
    assert assert_planes_match_traces(planes, pixels, traces, name) == 64
