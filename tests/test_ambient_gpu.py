"""The ambient pass (include/svr_ambient.h) on the MI355X.

The reference is tests/native/ambient_ref.cpp (ambient_ref.py), the scalar restatement of DESIGN C32-C37 that
test_ambient_ref.py pins on the CPU.  It is fed the depth and normal planes the HIP library itself holds, so every
comparison with it is on bit patterns, over the whole plane, with no tolerance.  Part 6 adds the scissor's and the staging's
edges and, without the restatement in between, the comparison with ambient_ref.ao64 under its own ties and bound."""
import numpy as np
import pytest

import __graft_entry__ as g
import ambient_ref as AR
import lighting_ref as LR
import svr_testlib as T

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
PATTERN = (0.25, 0.5, 0.75, 0.125)
OTHER_LIGHTING = ((0.35, 0.5, 0.45, 1.0), (0.6, 0.3, -0.7, 0.0), (1.0, 0.9, 0.8, 0.7))  # ambient, sun direction, sun colour
TUNE_NO_POLL = 16
GBUFFER = A.ATTR_NORMAL | A.ATTR_ALBEDO
SENTINEL = f32(7.0)  # no ambient factor: what the pass must leave outside the scissor
SCENE_PARAMS = dict(radius=0.6, bias=0.01, intensity=1.5, sharpness=0.05)


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])].tolist()} vs {want[tuple(np.argwhere(bad)[0])].tolist()}"


# ---------------------------------------------------------------- 1. random planes in caller tensors
@pytest.mark.parametrize("flags", [0, A.AMBIENT_NO_BLUR], ids=["blur", "no_blur"])
@pytest.mark.parametrize("scissor", [None, AR.ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_random_planes(hip, scissor, flags):
    torch = pytest.importorskip("torch")
    w, h = AR.PLANE
    depth, normal, inv_vp, ppu, ref = AR.plane_case(scissor, flags)
    AR.assert_plane_case_is_telling(ref, scissor)
    t_color = torch.full((h, w, 2), 0x3C003800, dtype=torch.int32, device="cuda")
    t_depth = torch.from_numpy(depth.copy()).cuda()
    t_normal = torch.from_numpy(normal.copy()).cuda()
    t_ao = torch.full((h, w), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = hip.create(w, h)
    r.bind_targets(t_color.data_ptr(), t_depth.data_ptr())
    r.bind_attribute_target(A.ATTR_NORMAL, t_normal.data_ptr())
    assert r.get_ambient_target() is None
    r.bind_ambient_target(t_ao.data_ptr())
    assert r.get_ambient_target() == t_ao.data_ptr()
    if scissor:
        r.set_scissor(*scissor)
    P = AR.PLANE_PARAMS
    r.ambient_pass(inv_vp.reshape(4, 4), P["radius"], ppu, P["bias"], P["intensity"], P["sharpness"], flags)
    raw = r.read_ambient_raw()  # (fences)
    out = t_ao.cpu().numpy()
    inside = AR.inside_of((h, w), scissor or (0, 0, w, h))
    AR.assert_planes(raw, ref["raw"], "the raw (a, 1/w) plane")  # zero outside the scissor on both sides
    AR.assert_planes(out, np.where(inside, ref["out"], SENTINEL), "the ambient target")
    AR.assert_planes(r.read_ambient(), out, "svr_read_ambient against the bound tensor")
    assert np.array_equal(AR.bits(t_depth.cpu().numpy()), AR.bits(depth)), "depth is read only"
    assert np.array_equal(AR.bits(t_normal.cpu().numpy()), AR.bits(normal)), "the normal plane is read only"
    assert (t_color.cpu().numpy() == 0x3C003800).all(), "colour is not touched"
    r.bind_ambient_target(None)
    assert r.get_ambient_target() is None, "nothing bound and no pass into a plane of the context's yet"
    r.close()


# ---------------------------------------------------------------- 2. a rendered G-buffer
def atrium(lib, w, h, fmt=A.COLOR_RGBA16F, options=()):
    r, scene, opaque, transparent = T.setup_sponza(lib, w, h, color_format=fmt)
    r.enable_attributes(GBUFFER)
    return r, scene, opaque, transparent


def camera_of(scene, h):
    return LR.inv_viewproj(scene.viewproj), GL.pixels_per_unit(np.array(scene.proj, f32).reshape(4, 4), h)


def ambient(r, scene, h, flags=0, **kw):
    inv_vp, ppu = camera_of(scene, h)
    p = dict(SCENE_PARAMS, **kw)
    r.ambient_pass(inv_vp.reshape(4, 4), p["radius"], ppu, p["bias"], p["intensity"], p["sharpness"], flags)


def reference(r, scene, h, flags=0, scissor=None, **kw):
    inv_vp, ppu = camera_of(scene, h)
    return AR.run_ref(r.read_depth(), r.read_attribute(A.ATTR_NORMAL), inv_vp, ppu=ppu, flags=flags, scissor=scissor, **dict(SCENE_PARAMS, **kw))


@pytest.mark.parametrize("flags", [0, A.AMBIENT_NO_BLUR], ids=["blur", "no_blur"])
def test_rendered_gbuffer(hip, flags):
    w, h = 160, 96
    r, scene, opaque, _ = atrium(hip, w, h)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    ambient(r, scene, h, flags)
    ref = reference(r, scene, h, flags)
    assert (ref["out"] < 1).mean() > 0.02 and (ref["out"] == 1).any(), "the scene has creases, and open ground"
    AR.assert_planes(r.read_ambient(), ref["out"], "the ambient target")
    AR.assert_planes(r.read_ambient_raw(), ref["raw"], "the raw plane")
    assert_color(r.read_color(), first["color"], "colour")
    assert np.array_equal(AR.bits(r.read_depth()), AR.bits(first["depth"])) and np.array_equal(r.read_ids(), first["ids"])
    for a, plane in first["attr"].items():
        assert np.array_equal(AR.bits(r.read_attribute(a)), AR.bits(plane)), a
    # a second pass under a scissor rewrites the scissor's pixels only
    scissor = (21, 9, 100, 71)
    r.set_scissor(*scissor)
    ambient(r, scene, h, flags, radius=0.3)
    inside = AR.inside_of((h, w), scissor)
    two = reference(r, scene, h, flags, scissor=scissor, radius=0.3)
    AR.assert_planes(r.read_ambient(), np.where(inside, two["out"], ref["out"]), "the ambient target after a pass under a scissor")
    assert (two["out"][inside] != ref["out"][inside]).any()
    r.close()


# ---------------------------------------------------------------- 3. the lighting pass takes the plane
@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8], ids=["rgba16f", "rgba8"])
def test_light_pass_with_a_plane_of_ones_is_the_light_pass(hip, fmt):
    torch = pytest.importorskip("torch")
    w, h = 160, 96
    r, scene, opaque, _ = atrium(hip, w, h, fmt)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    inv_vp = LR.inv_viewproj(scene.viewproj)
    r.light_pass(inv_vp, *OTHER_LIGHTING)
    off = r.read_color()
    ones = torch.ones((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_ambient_target(ones.data_ptr())
    r.set_light_ambient_occlusion(True)
    r.clear_color(PATTERN)
    r.light_pass(inv_vp, *OTHER_LIGHTING)
    assert_color(r.read_color(), off, "switch on, a plane of ones")
    half = torch.full((h, w), 0.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_ambient_target(half.data_ptr())
    r.light_pass(inv_vp, *OTHER_LIGHTING)
    assert (r.read_color() != off).any(), "a plane of halves is seen"
    r.set_light_ambient_occlusion(False)
    r.light_pass(inv_vp, *OTHER_LIGHTING)
    assert_color(r.read_color(), off, "switch off again")
    r.close()


@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8], ids=["rgba16f", "rgba8"])
def test_lit_colour_with_the_passes_plane(hip, fmt):
    w, h = 160, 96
    r, scene, opaque, _ = atrium(hip, w, h, fmt)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    before = r.read_color()
    depth, normal, albedo = r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO)
    inv_vp = LR.inv_viewproj(scene.viewproj)
    probe = LR.run_ref(depth, normal, albedo, inv_vp, *OTHER_LIGHTING)
    rng = np.random.default_rng(31)
    ys, xs = np.nonzero(probe["winner"] & np.all(np.isfinite(probe["position"]), axis=-1))
    pick = rng.integers(0, len(ys), 5)
    lights = np.zeros(5, A.POINT_LIGHT_DTYPE)
    lights["position"] = probe["position"][ys[pick], xs[pick]] + rng.normal(0, 0.3, (5, 3)).astype(f32)
    lights["radius"], lights["color"], lights["intensity"] = 6.0, rng.uniform(0.2, 1.0, (5, 3)).astype(f32), 2.0
    ambient(r, scene, h)
    ao = r.read_ambient()
    AR.assert_planes(ao, reference(r, scene, h)["out"], "the ambient target")
    r.set_light_ambient_occlusion(True)
    r.light_pass(inv_vp, *OTHER_LIGHTING, lights=lights)
    want = AR.run_light_ref(depth, normal, albedo, ao, inv_vp, *OTHER_LIGHTING, lights=lights)
    plain = LR.run_ref(depth, normal, albedo, inv_vp, *OTHER_LIGHTING, lights=lights)
    assert (LR.store(want["rgba"], fmt) != LR.store(plain["rgba"], fmt)).any(), "the factor shows in the stored colour"
    assert_color(r.read_color(), LR.expected_color(before, want, fmt), "lit with the pass's plane and five point lights")
    r.close()


def test_light_pass_without_a_plane_is_refused(hip):
    w, h = 64, 32
    r, scene, opaque, _ = atrium(hip, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    before = r.read_color()
    inv_vp = LR.inv_viewproj(scene.viewproj)
    r.set_light_ambient_occlusion(True)
    with pytest.raises(A.SvrError, match="no ambient target") as e:
        r.light_pass(inv_vp, *OTHER_LIGHTING)
    assert e.value.code == -1
    assert_color(r.read_color(), before, "a refused lighting pass changes nothing")
    with pytest.raises(A.SvrError, match="no ambient target"):
        r.read_ambient()
    ambient(r, scene, h)  # the context's plane now exists
    assert r.get_ambient_target()
    r.light_pass(inv_vp, *OTHER_LIGHTING)
    assert (r.read_color() != before).any()
    r.close()


# ---------------------------------------------------------------- 4. ordering
def test_replayed_behind_an_overflowing_pass(hip):
    """an ambient pass and the lighting pass that uses it, behind a G-buffer pass that overflows: both are void the first
    time and run in the replay, in call order, from the planes they were logged with"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, _ = atrium(hip, w, h)
        inv_vp = LR.inv_viewproj(scene.viewproj)
        ambient(r, scene, h, radius=0.2)  # the planes exist and hold another pass's values
        r.set_light_ambient_occlusion(True)
        r.sync()
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        ambient(r, scene, h)  # enqueued behind a pass that is still void
        r.light_pass(inv_vp, *OTHER_LIGHTING)
        frames[caps] = (r.read_ambient(), r.read_ambient_raw(), r.read_color(), r.get_stats().replayed_passes)
        if caps is None:
            ref = reference(r, scene, h)
            depth, normal, albedo = r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO)
            r.set_light_ambient_occlusion(False)
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, EMPTY)
            forward = r.read_color()
        r.close()
    assert frames[None][3] == 0 and frames[64][3] > 0
    assert (ref["out"] != 1).any(), "a pass that did not run again would show: the first one, over an empty G-buffer, wrote ones"
    lit = AR.run_light_ref(depth, normal, albedo, ref["out"], inv_vp, *OTHER_LIGHTING)
    for caps, what in ((None, "no overflow"), (64, "behind a replayed pass")):
        AR.assert_planes(frames[caps][0], ref["out"], "the ambient target, " + what)
        AR.assert_planes(frames[caps][1], ref["raw"], "the raw plane, " + what)
        assert_color(frames[caps][2], LR.expected_color(forward, lit, A.COLOR_RGBA16F), "the lit colour, " + what)


def test_not_replayed_in_front_of_an_overflowing_pass(hip):
    """G-buffer pass, ambient pass, then a pass that overflows: the ambient pass landed before the failing pass and the
    replay starts at that pass; its plane is what it wrote"""
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        r, scene, opaque, transparent = atrium(hip, w, h)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        ref = reference(r, scene, h)
        if caps is not None:
            r.set_option(A.OPT_QUEUE_CAPS, caps)  # (a fence: the first pass is done; the next one starts from tiny queues)
            r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        ambient(r, scene, h)
        r.set_depth_load_op(A.DEPTH_LOAD)
        r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), transparent)
        frames[caps] = (r.read_ambient(), r.read_ambient_raw(), r.read_color(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][3] == 0 and frames[64][3] > 0
    for caps, what in ((None, "no overflow"), (64, "in front of a replayed pass")):
        AR.assert_planes(frames[caps][0], ref["out"], "the ambient target, " + what)
        AR.assert_planes(frames[caps][1], ref["raw"], "the raw plane, " + what)
    assert_color(frames[64][2], frames[None][2], "the frame")


def test_a_deferred_clear_stays_deferred(hip):
    """the pass writes no colour: a clear in front of it is still taken by the geometry pass behind it"""
    w, h = 96, 64
    r, scene, opaque, _ = atrium(hip, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), EMPTY)
    want = r.read_color()
    r.clear_color(CLEAR)
    ambient(r, scene, h)
    r.draw_geometry(scene, np.ascontiguousarray(opaque[::3]), EMPTY)
    assert_color(r.read_color(), want, "clear, ambient pass, geometry pass")
    r.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals(hip):
    w, h = 64, 32
    r, scene, opaque, _ = atrium(hip, w, h)
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, EMPTY)
    with pytest.raises(A.SvrError, match="no ambient pass yet"):
        r.read_ambient_raw()
    ambient(r, scene, h)
    before = (r.read_ambient(), r.read_ambient_raw(), r.read_color())
    inv_vp, ppu = camera_of(scene, h)
    good = dict(inv_viewproj=inv_vp.reshape(4, 4), radius=0.5, pixels_per_unit=ppu, bias=0.01, intensity=1.0, sharpness=0.05, flags=0)
    nan, inf = float("nan"), float("inf")
    bad_m = inv_vp.reshape(4, 4).copy()
    bad_m[2][1] = nan
    inf_m = inv_vp.reshape(4, 4).copy()
    inf_m[0][0] = inf
    bad = [dict(radius=v) for v in (0.0, -1.0, nan, inf)] + [dict(pixels_per_unit=v) for v in (0.0, -3.0, nan, inf)] + \
          [dict(bias=v) for v in (-0.01, nan, inf)] + [dict(intensity=v) for v in (-1.0, nan, inf)] + \
          [dict(sharpness=v) for v in (-0.1, 1.0, 1.5, nan, inf)] + [dict(flags=2), dict(flags=A.AMBIENT_NO_BLUR | 4)] + \
          [dict(inv_viewproj=bad_m), dict(inv_viewproj=inf_m)]
    for kw in bad:
        with pytest.raises(A.SvrError) as e:
            r.ambient_pass(**dict(good, **kw))
        assert e.value.code == -1, kw
    assert hip.lib.svr_ambient_pass(r.h, None) == -1
    with pytest.raises(A.SvrError, match="16-byte aligned"):
        r.bind_ambient_target(r.get_ambient_target() + 4)
    r.set_row_interleave(2, 0)
    with pytest.raises(A.SvrError, match="svr_set_row_interleave") as e:
        r.ambient_pass(**good)
    assert e.value.code == -5
    r.set_row_interleave(1, 0)
    r.enable_attributes(A.ATTR_ALBEDO)  # the normal plane goes
    with pytest.raises(A.SvrError, match="SVR_ATTR_NORMAL") as e:
        r.ambient_pass(**good)
    assert e.value.code == -1
    AR.assert_planes(r.read_ambient(), before[0], "refused calls change nothing")
    AR.assert_planes(r.read_ambient_raw(), before[1], "nor the raw plane")
    assert_color(r.read_color(), before[2], "nor colour")
    r.close()


# ---------------------------------------------------------------- 6. scissor edges, alignment, specials, and the fp64 statement
def ambient_over(hip, depth, normal, inv_vp, ppu, scissor, flags, params=AR.PLANE_PARAMS):
    """one pass over caller-bound planes -> (the raw plane, the bound ambient tensor, which held SENTINEL everywhere)"""
    torch = pytest.importorskip("torch")
    h, w = depth.shape
    t_color = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda")
    t_depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=f32)).cuda()
    t_normal = torch.from_numpy(np.ascontiguousarray(normal, dtype=f32)).cuda()
    t_ao = torch.full((h, w), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = hip.create(w, h)
    r.bind_targets(t_color.data_ptr(), t_depth.data_ptr())
    r.bind_attribute_target(A.ATTR_NORMAL, t_normal.data_ptr())
    r.bind_ambient_target(t_ao.data_ptr())
    if scissor:
        r.set_scissor(*scissor)
    r.ambient_pass(np.asarray(inv_vp, f32).reshape(4, 4), params["radius"], ppu, params["bias"], params["intensity"], params["sharpness"], flags)
    raw = r.read_ambient_raw()  # (fences)
    out = t_ao.cpu().numpy()
    r.close()
    return raw, out


def assert_pass_is(raw, out, ref, scissor, what):
    """bit patterns over the whole plane: the raw plane zero and the target untouched outside the scissor"""
    inside = AR.inside_of(out.shape, scissor)
    AR.assert_planes(raw, ref["raw"], f"{what}: the raw (a, 1/w) plane")
    AR.assert_planes(out, np.where(inside, ref["out"], SENTINEL), f"{what}: the ambient target")


@pytest.mark.parametrize("flags", [0, A.AMBIENT_NO_BLUR], ids=["blur", "no_blur"])
@pytest.mark.parametrize("name", list(AR.EDGE_SCISSORS))
def test_degenerate_and_seam_scissors(hip, name, flags):
    scissor = AR.EDGE_SCISSORS[name]
    depth, normal, inv_vp, ppu, _ = AR.plane_case(None, 0)
    ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, flags=flags, scissor=scissor, **AR.PLANE_PARAMS)
    assert (ref["kind"] != 0).sum() == scissor[2] * scissor[3]
    raw, out = ambient_over(hip, depth, normal, inv_vp, ppu, scissor, flags)
    assert_pass_is(raw, out, ref, scissor, name)


@pytest.mark.parametrize("scissor", [AR.ODD_SCISSOR, AR.EDGE_SCISSORS["one_into_a_second_tile_at_the_end"]], ids=["odd_scissor", "at_the_end"])
def test_nothing_outside_the_scissor_is_read(hip, scissor):
    """every texel outside the scissor holds what would show if it were read: NaN or a near, occluding depth, a NaN normal"""
    depth, normal, inv_vp, ppu, _ = AR.plane_case(None, 0)
    ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, scissor=scissor, **AR.PLANE_PARAMS)
    bad_depth, bad_normal = AR.poisoned_outside(depth, normal, scissor)
    shown = AR.run_ref(np.nan_to_num(bad_depth, nan=0.9), normal, inv_vp, ppu=ppu, scissor=None, **AR.PLANE_PARAMS)
    inside = AR.inside_of(depth.shape, scissor)
    assert (shown["out"][inside] != ref["out"][inside]).mean() > 0.02, "a pass that read past the scissor would differ"
    raw, out = ambient_over(hip, bad_depth, bad_normal, inv_vp, ppu, scissor, 0)
    assert_pass_is(raw, out, ref, scissor, "planes poisoned outside the scissor")


@pytest.mark.parametrize("w", [64, 65, 66, 67])
def test_alignment_parities(hip, w):
    """row starts and scissor origins at every residue of a 16-byte group: with the width and the origin, every row of the
    staging takes the 16-byte load, none does, or some rows do, and the right edge falls at every place inside a group"""
    depth, normal, inv_vp, ppu = AR.small_plane(w)
    h = depth.shape[0]
    vector_rows = set()
    for x0 in range(5):
        scissor = (x0, 0, w - x0, h)
        vector_rows.add(sum((y * w + x0) % 4 == 0 for y in range(h)))
        ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, scissor=scissor, **AR.PLANE_PARAMS)
        assert (ref["out"][:, x0:] < 1).mean() > 0.1 and (ref["kind"] == AR.CAPPED).any()
        raw, out = ambient_over(hip, depth, normal, inv_vp, ppu, scissor, 0)
        assert_pass_is(raw, out, ref, scissor, f"width {w}, origin {x0}")
    assert vector_rows == ({0, h} if w % 4 == 0 else {0, h // 2} if w % 2 == 0 else {h // 4})  # rows whose start is 16-byte aligned


def assert_bits_or_nan(got, want, what):
    nan = np.isnan(want)
    AR.assert_planes(np.where(nan, f32(0), got), np.where(nan, f32(0), want), what)
    assert np.isnan(got[nan]).all(), f"{what}: a NaN of the reference's is a NaN"


@pytest.mark.parametrize("flags", [0, A.AMBIENT_NO_BLUR], ids=["blur", "no_blur"])
def test_specials(hip, flags):
    """infinite, negative, -0.0 and subnormal depths, a normal w of -0.0, infinite and underflowing normals: a kernel built to
    flush fp32 denormals, or whose max prefers the other operand, differs from the contract here"""
    depth, normal, inv_vp, ppu = AR.special_plane()
    assert np.isinf(depth).any() and (depth < 0).any() and ((depth > 0) & (depth < 1e-38)).any() and not np.isnan(depth).any()
    assert (AR.bits(normal[..., 3]) == 0x80000000).any() and np.isinf(normal).any()
    ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, flags=flags, **AR.PLANE_PARAMS)
    tiny = (depth > 0) & (depth < 1e-38) & (ref["kind"] != AR.NO_SURFACE)
    assert tiny.any() and (ref["raw"][..., 1][tiny] != 0).all(), "a subnormal depth is a surface"
    raw, out = ambient_over(hip, depth, normal, inv_vp, ppu, None, flags)
    for c, part in enumerate(("a", "1/w")):
        assert_bits_or_nan(raw[..., c], ref["raw"][..., c], f"specials: the raw plane's {part}")
    assert_bits_or_nan(out, ref["out"], "specials: the ambient target")


@pytest.mark.parametrize("scissor", [None, AR.ODD_SCISSOR], ids=["whole", "odd_scissor"])
def test_behind_the_eye_plane(hip, scissor):
    depth, normal = AR.plane_case(None, 0)[:2]
    inv_vp, ppu = AR.behind_the_eye(*AR.PLANE)
    ref = AR.run_ref(depth, normal, inv_vp, ppu=ppu, scissor=scissor, **AR.PLANE_PARAMS)
    AR.assert_behind_the_eye(ref, scissor or (0, 0) + AR.PLANE)
    raw, out = ambient_over(hip, depth, normal, inv_vp, ppu, scissor, 0)
    assert_pass_is(raw, out, ref, scissor or (0, 0) + AR.PLANE, "h.w < 0 on the left")


@pytest.mark.parametrize("case", ["random_planes", "crease"])
def test_against_the_fp64_statement(hip, case):
    """the HIP library against ambient_ref.ao64 itself, with its ties and its bound: no CPU restatement in between"""
    if case == "random_planes":
        depth, normal, inv_vp, ppu, _ = AR.plane_case(AR.ODD_SCISSOR, 0)
        scissor, params, st = AR.ODD_SCISSOR, AR.PLANE_PARAMS, AR.plane_statement(AR.ODD_SCISSOR)
    else:
        depth, normal, inv_vp, ppu, _ = AR.analytic_scene(case)
        scissor, params, st = (0, 0) + AR.SCENE, AR.SCENE_PARAMS, AR.scene_statement(case)
    AR.assert_statement_is_telling(st, 0, scissor)
    AR.assert_statement_is_telling(st, AR.NO_BLUR, scissor)
    raw, out = ambient_over(hip, depth, normal, inv_vp, ppu, scissor, 0, params)
    for flags, plane, what in ((0, out, "the ambient target"), (AR.NO_BLUR, raw[..., 0], "the raw plane's a")):
        worst, at, beyond = AR.compare64(plane, st, flags, scissor)
        print(f"{case}, {what}: largest |HIP - ao64| / bound = {worst:.4f} at (y, x) = {at}")
        assert beyond == 0, f"{case}, {what}: {beyond} compared pixels beyond the bound, the worst {worst:.3g} bounds off at (y, x) = {at}"
    keep = AR.inside_of(out.shape, scissor) & ~st["tie_a"]
    assert np.allclose(raw[..., 1][keep], st["hw"][keep], rtol=16 * AR.EPS, atol=0)
