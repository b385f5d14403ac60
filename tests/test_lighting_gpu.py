"""The deferred lighting pass (include/svr_lighting.h) on the MI355X.

The reference is tests/native/light_ref.cpp (lighting_ref.py): a scalar program that visits every light at every pixel,
pinned to the CPU oracle by test_lighting_ref.py.  It is fed the G-buffer the HIP library itself wrote (the planes are
checked against the oracle by test_attributes_gpu.py), so every comparison here is on bit patterns, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import lighting_ref as LR
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
CLEAR = (1.0, 1.0, 1.0, 1.0)
PATTERN = (0.25, 0.5, 0.75, 0.125)  # a colour no lit pixel holds (alpha is not 1): what the pass must leave alone
OTHER_LIGHTING = ((0.05, 0.2, 0.15, 1.0), (0.6, 0.3, -0.7, 0.0), (1.0, 0.9, 0.8, 0.7))  # ambient, sun direction, sun colour
TUNE_NO_POLL = 16
GBUFFER = A.ATTR_NORMAL | A.ATTR_ALBEDO


def atrium(lib, w, h, fmt=A.COLOR_RGBA16F, subset=None, options=(), attrs=GBUFFER):
    """the atrium's opaque objects (every pixel has a winner; subset: a slice of them, which leaves background pixels)
    drawn into a fresh context with the G-buffer planes enabled -> (renderer, scene, objects)"""
    r, scene, opaque, _ = T.setup_sponza(lib, w, h, color_format=fmt)
    for k, v in options:
        r.set_option(k, v)
    if attrs and lib.has_attributes:
        r.enable_attributes(attrs)
    op = opaque if subset is None else np.ascontiguousarray(opaque[subset])
    r.clear_color(CLEAR)
    r.draw_geometry(scene, op, EMPTY)
    return r, scene, op


def gbuffer(r):
    return r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO)


def relight(r, scene, lighting=None, **kw):
    ambient, sun_dir, sun_color = lighting if lighting is not None else LR.lighting_of(scene)
    r.light_pass(LR.inv_viewproj(scene.viewproj), ambient, sun_dir, sun_color, **kw)


def reference(r, scene, lighting=None, **kw):
    ambient, sun_dir, sun_color = lighting if lighting is not None else LR.lighting_of(scene)
    depth, normal, albedo = gbuffer(r)
    return LR.run_ref(depth, normal, albedo, LR.inv_viewproj(scene.viewproj), ambient, sun_dir, sun_color, **kw)


def make_lights(n, ref, seed, diameter=70.0, smallest=0.05):
    """n seeded lights near the surfaces the reference found: radii log-uniform from under one tile's world footprint to
    the whole scene; light 0 sits exactly on a surface point, light 1 (if any) has a radius that reaches nothing"""
    rng = np.random.default_rng(seed)
    L = np.zeros(n, A.POINT_LIGHT_DTYPE)
    if n == 0:
        return L
    ok = ref["winner"] & np.all(np.isfinite(ref["position"]), axis=-1)
    ys, xs = np.nonzero(ok)
    pick = rng.integers(0, len(ys), n)
    base = ref["position"][ys[pick], xs[pick]]
    L["position"] = base + rng.normal(0, 0.4, (n, 3)).astype(f32)
    L["radius"] = (10.0 ** rng.uniform(np.log10(smallest), np.log10(diameter), n)).astype(f32)
    L["color"] = rng.uniform(0.2, 1.0, (n, 3)).astype(f32)
    L["intensity"] = rng.uniform(0.5, 4.0, n).astype(f32)
    L["position"][0], L["radius"][0] = base[0], 2.0
    if n > 1:
        L["position"][1], L["radius"][1] = base[1] + np.array([0.11, 0.23, 0.17], f32), 1e-3
    if n > 2:
        L["radius"][2] = diameter
    return L


def assert_color(got, want, what):
    bad = np.any(got != want, axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])].tolist()} vs {want[tuple(np.argwhere(bad)[0])].tolist()}"


# ---------------------------------------------------------------- 1. relighting with no lights is the forward pass
@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8])
def test_relight_equals_forward(hip, oracle, fmt):
    w, h = 160, 96
    r, scene, op = atrium(hip, w, h, fmt)
    forward = r.read_color()
    relight(r, scene)
    assert_color(r.read_color(), forward, "relit with the scene's lighting against the forward pass")
    o, oscene, oop = atrium(oracle, w, h, fmt)
    assert_color(forward, o.read_color(), "forward pass against the oracle")
    relight(r, scene, OTHER_LIGHTING)
    changed = r.read_color()
    oscene.ambient_color, oscene.sunlight_direction, oscene.sunlight_color = (A._f4(v) for v in OTHER_LIGHTING)
    o.clear_color(CLEAR)
    o.draw_geometry(oscene, oop, EMPTY)
    want = o.read_color()
    o.close()
    assert not np.array_equal(want, forward)
    assert_color(changed, want, "relit under another sun and ambient against the oracle's frame under them")
    assert r.read_light_tiles().tolist() == [0] * (5 * 3)
    r.close()


def test_relight_with_caller_bound_tensors(hip):
    torch = pytest.importorskip("torch")
    w, h = 160, 96
    r, scene, op = atrium(hip, w, h)
    forward = r.read_color()
    relight(r, scene, OTHER_LIGHTING)
    want = r.read_color()
    color = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda")
    depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    normal = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    albedo = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    r.bind_attribute_target(A.ATTR_NORMAL, normal.data_ptr())
    r.bind_attribute_target(A.ATTR_ALBEDO, albedo.data_ptr())
    r.clear_color(CLEAR)
    r.draw_geometry(scene, op, EMPTY)
    r.sync()
    assert_color(color.cpu().numpy().view(np.uint16).reshape(h, w, 4), forward, "forward pass into bound tensors")
    relight(r, scene, OTHER_LIGHTING)
    r.sync()
    assert_color(color.cpu().numpy().view(np.uint16).reshape(h, w, 4), want, "relit in bound tensors")
    r.close()


# ---------------------------------------------------------------- 2. against light_ref, every pixel
CASES = {
    "lights_0": dict(size=(96, 64), n=0),
    "lights_1": dict(size=(96, 64), n=1),
    "lights_33": dict(size=(96, 64), n=33),
    "lights_65": dict(size=(96, 64), n=65),
    "lights_300": dict(size=(96, 64), n=300),
    "rgba8": dict(size=(96, 64), n=65, fmt=A.COLOR_RGBA8),
    "partial_tiles_33x35": dict(size=(33, 35), n=65),
    "160x96": dict(size=(160, 96), n=300),
    "odd_scissor": dict(size=(160, 96), n=65, scissor=(37, 21, 101, 57)),
    "interleave_3_0": dict(size=(160, 96), n=65, interleave=(3, 0)),
    "interleave_3_2": dict(size=(160, 96), n=65, interleave=(3, 2)),
    "background": dict(size=(96, 64), n=33, subset=slice(0, None, 3), pattern=False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_light_ref(hip, name):
    c = CASES[name]
    (w, h), fmt = c["size"], c.get("fmt", A.COLOR_RGBA16F)
    r, scene, op = atrium(hip, w, h, fmt, subset=c.get("subset"))
    unlit = reference(r, scene)
    lights = make_lights(c["n"], unlit, seed=100 + c["n"])
    ref = reference(r, scene, lights=lights)
    if c.get("pattern", True):
        r.clear_color(PATTERN)  # the whole frame: what is not owned must keep it
    before = r.read_color()
    if "scissor" in c:
        r.set_scissor(*c["scissor"])
    if "interleave" in c:
        r.set_row_interleave(*c["interleave"])
    relight(r, scene, lights=lights)
    got = r.read_color()
    owned = LR.owned_mask(w, h, c.get("scissor"), c.get("interleave", (1, 0)))
    lit = ref["winner"] & owned
    assert lit.sum() >= 512
    if c["n"]:
        assert (LR.store(ref["rgba"], fmt) != LR.store(unlit["rgba"], fmt))[lit].any(), "the lights must reach an owned pixel"
    if name == "background":
        assert (~ref["winner"]).sum() >= 256, "the case needs background pixels"
    assert_color(got, LR.expected_color(before, ref, fmt, owned), name)
    r.close()


def near_clip_wall(lib, w=80, h=60):
    """the wall of scenarios.near_clip_wall: the camera nearly touches it, and it crosses the near plane and the guard
    band -> (Rig, scene, objects)"""
    rig = SC.Rig(lib, w, h)
    img = rig.r.create_image(S.checkerboard_32(), mipmapped=True)
    pos = [(-50, -40, -3.0), (60, -40, 1.0), (60, 45, 1.0), (-50, 45, -3.0)]
    mesh = rig.r.upload_mesh(SC.QUAD_IDX, SC.make_vertices(pos, [(0.3, 0.5, 1)] * 4, [(0, 0), (9, 0), (9, 7), (0, 7)]))
    mat = rig.material(image=img, sampler=rig.trilinear)
    scene = S.scene_data_struct((0.0, 0.0, 0.0), 0.1, -0.2, w, h)
    return rig, scene, [SC.render_object(mesh, mat, 0, 6, origin=(0, 0, -5), extents=(1, 1, 1))]


def test_near_clip_scene_against_light_ref(hip):
    rig, scene, objects = near_clip_wall(hip)
    r = rig.r
    r.enable_attributes(GBUFFER)
    rig.draw(scene, objects)
    before = r.read_color()
    lights = make_lights(33, reference(r, scene), seed=7)
    ref = reference(r, scene, lights=lights)
    assert ref["winner"].sum() >= 1024 and np.isfinite(ref["position"][ref["winner"]]).all()
    relight(r, scene, lights=lights)
    assert_color(r.read_color(), LR.expected_color(before, ref, A.COLOR_RGBA16F), "near_clip_wall")
    r.close()


def test_synthetic_planes_with_non_finite_positions(hip):
    """planes written by the caller: a winner flag over depth 0 under a projective inverse whose w is the depth, so 1/w is
    inf and the position inf or NaN: such pixels take the sun's term alone, bit for bit as the reference"""
    torch = pytest.importorskip("torch")
    w, h = 70, 45
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.05, 1.0, (h, w)).astype(f32)
    depth[rng.random((h, w)) < 0.25] = 0.0
    normal = rng.normal(0, 1, (h, w, 4)).astype(f32)
    albedo = rng.uniform(0, 1, (h, w, 4)).astype(f32)
    flag = rng.random((h, w))
    albedo[..., 3] = np.where(flag < 0.7, 1.0, np.where(flag < 0.85, 0.0, 0.5)).astype(f32)
    inv_vp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], f32)  # columns: p = (xn, yn, 1) / depth
    lights = np.zeros(33, A.POINT_LIGHT_DTYPE)
    lights["position"] = rng.uniform(-4, 4, (33, 3)).astype(f32) + np.array([0, 0, 5], f32)
    lights["radius"] = (10.0 ** rng.uniform(-0.5, 1.5, 33)).astype(f32)
    lights["color"], lights["intensity"] = rng.uniform(0.2, 1, (33, 3)).astype(f32), rng.uniform(0.5, 3, 33).astype(f32)
    shadow = rng.uniform(0, 0.5, (16, 24)).astype(f32)
    view = GL.camera_view((0.0, 0.0, -2.0), 0.0, float(GL.radians(180.0)))
    shadow_vp = LR.m16(GL.scene_data(view, 24, 16)[2])
    lighting = OTHER_LIGHTING
    ref = LR.run_ref(depth, normal, albedo, inv_vp, *lighting, lights=lights, shadow=shadow, shadow_vp=shadow_vp, bias=1e-4)
    win = ref["winner"]
    bad_p = win & ~np.all(np.isfinite(ref["position"]), axis=-1)
    assert bad_p.sum() >= 256 and (win & ~bad_p).sum() >= 256 and (~win).sum() >= 256
    t = {k: torch.from_numpy(v).cuda() for k, v in (("depth", depth), ("normal", normal), ("albedo", albedo), ("shadow", shadow))}
    before = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4)).copy()
    color = torch.from_numpy(before.view(np.int32).reshape(h, w, 2).copy()).cuda()
    torch.cuda.synchronize()
    r = hip.create(w, h)
    r.bind_targets(color.data_ptr(), t["depth"].data_ptr())
    r.bind_attribute_target(A.ATTR_NORMAL, t["normal"].data_ptr())
    r.bind_attribute_target(A.ATTR_ALBEDO, t["albedo"].data_ptr())
    r.light_pass(inv_vp, *lighting, lights=lights, shadow_ptr=t["shadow"].data_ptr(), shadow_size=(24, 16), shadow_viewproj=shadow_vp,
                 shadow_bias=1e-4)
    r.sync()
    got = color.cpu().numpy().view(np.uint16).reshape(h, w, 4)
    assert_color(got, LR.expected_color(before, ref, A.COLOR_RGBA16F), "synthetic planes")
    for k, v in (("depth", depth), ("normal", normal), ("albedo", albedo)):
        assert np.array_equal(t[k].cpu().numpy().view(np.uint32), v.view(np.uint32)), k
    r.close()


# ---------------------------------------------------------------- 3. the shadow map
FLOOR_X, FLOOR_Z = (-12.0, 12.0), (-20.0, 4.0)
SHADOW_SIZE = (64, 48)
SHADOW_BIAS = 2e-5
# the camera the shadow map is drawn from: (position, pitch, yaw)
SHADOW_CAMERAS = {
    "covers_the_frame": ((0.0, 30.0, -8.0), -1.35, 0.0),
    "partly_outside": ((0.0, 8.0, -2.0), -1.1, 0.0),
    "behind_the_light": ((0.0, 3.0, -6.0), -0.35, 0.0),  # the floor nearer than z = -6 is behind it: q.w <= 0
}


def floor_and_box(lib, w, h):
    """a floor (y = 0) and a box above it -> (Rig, objects)"""
    rig = SC.Rig(lib, w, h)
    (x0, x1), (z0, z1) = FLOOR_X, FLOOR_Z
    floor = SC.make_vertices([(x0, 0, z1), (x1, 0, z1), (x1, 0, z0), (x0, 0, z0)], [(0, 1, 0)] * 4, [(0, 0), (6, 0), (6, 6), (0, 6)],
                             [(0.8, 0.7, 0.6, 1)] * 4)
    mf = rig.r.upload_mesh(SC.QUAD_IDX, floor)
    cube = S.cube_mesh()
    mc = rig.r.upload_mesh(cube.indices, cube.vertices)
    mat = rig.material(image=rig.checker, sampler=rig.linear)
    world = GL.scale(GL.translate(GL.identity(), (0.5, 1.75, -7.0)), (2.5, 1.5, 2.5))
    objects = SC.objs([SC.render_object(mf, mat, 0, 6, extents=(12, 0, 12), origin=(0, 0, -8)),
                       SC.render_object(mc, mat, 0, cube.indices.size, transform=world, origin=(0, 0, 0), extents=(0.5, 0.5, 0.5))])
    return rig, objects


def shadow_scene(which):
    pos, pitch, yaw = SHADOW_CAMERAS[which]
    return S.scene_data_struct(pos, pitch, yaw, *SHADOW_SIZE)


@pytest.mark.parametrize("which", sorted(SHADOW_CAMERAS))
def test_shadow_map_from_a_depth_only_pass(hip, which):
    w, h = 160, 96
    light_rig, light_objects = floor_and_box(hip, *SHADOW_SIZE)
    sscene = shadow_scene(which)
    light_rig.r.draw_depth(sscene, light_objects)
    light_rig.r.sync()
    shadow = light_rig.r.read_depth()
    shadow_ptr = light_rig.r.get_targets()[1]
    assert (shadow > 0).sum() >= 256
    rig, objects = floor_and_box(hip, w, h)
    r = rig.r
    r.enable_attributes(GBUFFER)
    scene = S.scene_data_struct((0.0, 2.5, 3.0), -0.12, 0.0, w, h)
    rig.draw(scene, objects)
    before = r.read_color()
    lights = make_lights(33, reference(r, scene), seed=3, diameter=30.0)
    kw = dict(lights=lights, shadow_viewproj=LR.m16(sscene.viewproj))
    ref = reference(r, scene, shadow=shadow, bias=SHADOW_BIAS, shadow_vp=kw["shadow_viewproj"], lights=lights)
    relight(r, scene, shadow_ptr=shadow_ptr, shadow_size=SHADOW_SIZE, shadow_bias=SHADOW_BIAS, **kw)
    got = r.read_color()
    floor = ref["winner"] & (np.abs(ref["position"][..., 1]) < 1e-2)
    # the reference's own classification, and where its positions fall in the map (float64: counts only)
    p = np.concatenate([ref["position"].astype(np.float64), np.ones((h, w, 1))], axis=-1)
    q = p @ np.asarray(kw["shadow_viewproj"], np.float64).reshape(4, 4)  # column-major [col][row]: q_row = sum_col p_col m[col][row]
    with np.errstate(all="ignore"):
        inside = (q[..., 3] > 0) & (np.abs(q[..., 0] / q[..., 3]) < 1) & (np.abs(q[..., 1] / q[..., 3]) < 1)
    counts = {"shadowed": int((floor & ref["shadowed"]).sum()), "unshadowed": int((floor & ~ref["shadowed"]).sum()),
              "outside": int((floor & ~inside & (q[..., 3] > 0)).sum()), "behind": int((floor & (q[..., 3] <= 0)).sum())}
    print(which, counts)
    assert floor.sum() >= 2048 and counts["unshadowed"] > 0
    if which != "behind_the_light":
        assert counts["shadowed"] > 0
    if which == "covers_the_frame":
        assert counts["outside"] == 0 and counts["behind"] == 0
    if which == "partly_outside":
        assert counts["outside"] >= 256
    if which == "behind_the_light":
        assert counts["behind"] >= 256
    assert not ref["shadowed"][floor & ~inside].any()
    assert_color(got, LR.expected_color(before, ref, A.COLOR_RGBA16F), which)
    r.close()
    light_rig.r.close()


# ---------------------------------------------------------------- 4. culling is real and exact
def test_tile_counts_against_float64_geometry(hip):
    torch = pytest.importorskip("torch")
    w, h, n = 160, 96, 300
    r, scene, op = atrium(hip, w, h)
    depth, normal, albedo = gbuffer(r)
    albedo[32:64, 64:96] = 0.0  # tile (2, 1) loses its winners
    ta = torch.from_numpy(albedo).cuda()
    torch.cuda.synchronize()
    r.bind_attribute_target(A.ATTR_ALBEDO, ta.data_ptr())
    lights = make_lights(n, reference(r, scene), seed=100 + n)
    ref = reference(r, scene, lights=lights)
    before = r.read_color()
    relight(r, scene, lights=lights)
    counts = r.read_light_tiles()
    assert_color(r.read_color(), LR.expected_color(before, ref, A.COLOR_RGBA16F), "300 lights, one tile without winners")
    assert counts.shape == (15,)
    pos = ref["position"].astype(np.float64)
    lp, lr = lights["position"].astype(np.float64), lights["radius"].astype(np.float64)
    total_lo = 0
    for ty in range(3):
        for tx in range(5):
            k = int(counts[ty * 5 + tx])
            win = ref["winner"][32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32]
            if not win.any():
                assert (tx, ty) == (2, 1) and k == 0
                continue
            p = pos[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32][win]
            d2 = ((p[:, None, :] - lp[None, :, :]) ** 2).sum(-1)
            reached = (d2 < (lr * lr)[None, :] * (1 - 1e-5)).any(0)  # (the margin keeps float32 ties out of the lower bound)
            gap = np.maximum(np.maximum(p.min(0)[None, :] - lp, lp - p.max(0)[None, :]), 0.0)
            near = np.sqrt((gap ** 2).sum(-1)) <= 1.01 * lr
            assert reached.sum() <= k <= near.sum(), f"tile ({tx}, {ty}) kept {k} lights: at least {int(reached.sum())} reach a pixel, {int(near.sum())} are near its box"
            total_lo += int(reached.sum())
    assert total_lo > 0 and counts.sum() < 14 * n * 3 // 4, "culling must drop a good part of the lights"
    r.close()


# ---------------------------------------------------------------- 5. ordering
def test_replayed_after_a_queue_overflow(hip):
    w, h = 160, 96
    frames = {}
    for caps in (None, 64):
        options = () if caps is None else ((A.OPT_QUEUE_CAPS, caps), (A.OPT_TUNING, TUNE_NO_POLL))
        r, scene, opaque, _ = T.setup_sponza(hip, w, h)
        for k, v in options:
            r.set_option(k, v)
        r.enable_attributes(GBUFFER)
        if caps is None:
            r.clear_color(CLEAR)
            r.draw_geometry(scene, opaque, EMPTY)
            frames["lights"] = make_lights(65, reference(r, scene), seed=11)
        r.clear_color(CLEAR)
        r.draw_geometry(scene, opaque, EMPTY)
        relight(r, scene, OTHER_LIGHTING, lights=frames["lights"])  # enqueued behind a pass that is still void
        frames[caps] = (r.read_color(), r.read_light_tiles(), r.get_stats().replayed_passes)
        r.close()
    assert frames[None][2] == 0 and frames[64][2] > 0
    assert_color(frames[64][0], frames[None][0], "light pass behind a replayed pass")
    assert np.array_equal(frames[64][1], frames[None][1])


def test_a_deferred_clear_lands_before_the_pass(hip):
    w, h = 96, 64
    r, scene, op = atrium(hip, w, h, subset=slice(0, None, 3))
    lights = make_lights(33, reference(r, scene), seed=13)
    ref = reference(r, scene, lights=lights)
    assert (~ref["winner"]).sum() >= 256 and ref["winner"].sum() >= 256
    r.clear_color(PATTERN)  # deferred: no pass has taken it
    relight(r, scene, lights=lights)
    got = r.read_color()
    cleared = np.broadcast_to(LR.store(np.array(PATTERN, f32), A.COLOR_RGBA16F), (h, w, 4))
    assert_color(got, LR.expected_color(cleared, ref, A.COLOR_RGBA16F), "clear, then light pass")
    r.close()


# ---------------------------------------------------------------- 6. nothing else moves
def test_nothing_else_moves(hip):
    w, h = 160, 96
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h)
    r.enable_attributes(A.ATTR_ALL)
    r.enable_ids()
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)
    first = {"color": r.read_color(), "depth": r.read_depth(), "ids": r.read_ids(),
             "attr": {a: r.read_attribute(a) for a in (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO)}}
    lights = make_lights(65, reference(r, scene), seed=17)
    relight(r, scene, OTHER_LIGHTING, lights=lights)
    assert not np.array_equal(r.read_color(), first["color"])
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    assert np.array_equal(r.read_ids(), first["ids"])
    for a, plane in first["attr"].items():
        assert np.array_equal(r.read_attribute(a).view(np.uint32), plane.view(np.uint32)), a
    r.clear_color(CLEAR)
    r.draw_geometry(scene, opaque, transparent)  # a forward pass after it is what it was
    assert_color(r.read_color(), first["color"], "forward pass after a light pass")
    assert np.array_equal(r.read_depth().view(np.uint32), first["depth"].view(np.uint32))
    r.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(hip):
    w, h = 64, 32
    r = hip.create(w, h)
    ident = np.eye(4, dtype=f32)
    args = (ident, (0.1,) * 4, (0, 1, 0, 1), (1,) * 4)
    r.clear_color(PATTERN)
    before = r.read_color()
    for mask in (0, A.ATTR_NORMAL, A.ATTR_ALBEDO):  # missing planes
        r.enable_attributes(mask)
        with pytest.raises(A.SvrError, match="SVR_ATTR_NORMAL and SVR_ATTR_ALBEDO") as e:
            r.light_pass(*args)
        assert e.value.code == -1
    r.enable_attributes(GBUFFER)
    one = np.zeros(1, A.POINT_LIGHT_DTYPE)
    one["radius"] = 1.0
    r.light_pass(*args, lights=one)  # fine
    too_many = np.zeros(A.MAX_LIGHTS + 1, A.POINT_LIGHT_DTYPE)
    too_many["radius"] = 1.0
    with pytest.raises(A.SvrError, match="SVR_MAX_LIGHTS"):
        r.light_pass(*args, lights=too_many)
    r.light_pass(*args, lights=too_many[:A.MAX_LIGHTS])  # the most there can be
    for bad in (0.0, -1.0, np.nan, np.inf):
        three = np.zeros(3, A.POINT_LIGHT_DTYPE)
        three["radius"] = (1.0, 2.0, bad)
        with pytest.raises(A.SvrError, match="radius"):
            r.light_pass(*args, lights=three)
    p = A.SvrLightPass()
    p.n_lights = 1  # with a null array
    assert hip.lib.svr_light_pass(r.h, A.C.byref(p)) == -1
    for size in ((0, 16), (16, 0)):
        with pytest.raises(A.SvrError, match="shadow map"):
            r.light_pass(*args, shadow_ptr=r.get_targets()[1], shadow_size=size, shadow_viewproj=ident)
    assert_color(r.read_color(), before, "refused calls and passes over a G-buffer without winners change nothing")
    r.close()
