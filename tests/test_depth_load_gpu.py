"""The depth loadOp (include/svr_load.h) on the MI355X.

A pass under SVR_DEPTH_LOAD has no oracle of its own: the CPU oracle always clears.  What ties it to the oracle is that a
frame drawn in two passes, the second one over the depth the first one left, must be the frame drawn in one — and
test_parity_gpu.py ties that one to the oracle.  Besides that: arbitrary loaded depth through caller-bound tensors
(ties and one-ulp neighbours of the pass's own depth), the deferred chain the feature exists for, the replay after a
queue overflow, and the refusals.  Every comparison is on bit patterns, with no tolerance."""
import numpy as np
import pytest

import __graft_entry__ as g
import lighting_ref as LR
import scenarios as SC
import svr_testlib as T
from test_ids_gpu import TUNE_NO_SPLIT

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu
f32 = np.float32

EMPTY = np.zeros(0, A.RENDER_OBJECT_DTYPE)
TUNE_NO_POLL = 16  # SVR_OPT_TUNING bit (csrc/svr_device.h)
GBUFFER = A.ATTR_NORMAL | A.ATTR_ALBEDO
ODD_SCISSOR = (37, 21, 101, 57)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _objects(a):
    if a is None:
        return EMPTY
    return np.ascontiguousarray(a, dtype=A.RENDER_OBJECT_DTYPE).reshape(-1)


def assert_same(a, b, what, keys=("color", "depth", "rgba8"), where=None):
    for key in keys:
        x, y = a[key], b[key]
        if where is not None:
            sel = where if x.ndim == 2 else where[..., None]
            x, y = np.where(sel, x, 0), np.where(sel, y, 0)
        T.assert_images_identical(x, y, f"{what}: {key}")


def run(lib, name, mp, plan, options=(), setup=None):
    """Scenario `name` (or a scene builder) with its draw_geometry call handed to plan(r, scene, opaque, transparent, draw,
    extra) -> stats; `extra` joins the frame T._finish returns."""
    orig_draw, orig_finish = A.Renderer.draw_geometry, T._finish
    extra = {}

    def draw(self, scene, opaque, transparent=None):
        for k, v in options:
            self.set_option(k, v)
        if setup is not None:
            setup(self)
        return plan(self, scene, _objects(opaque), _objects(transparent), orig_draw, extra)

    def finish(r, stats=None):
        out = orig_finish(r, stats)
        out.update(extra)
        return out

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        m.setattr(T, "_finish", finish)
        return SC.SCENARIOS[name](lib) if isinstance(name, str) else name(lib)


def one_pass(r, scene, op, tr, draw, extra):
    return draw(r, scene, op, tr)


def two_passes(r, scene, op, tr, draw, extra):
    """the opaque objects under CLEAR (the scenario's clear_color rides in this pass), then the transparent ones under LOAD"""
    draw(r, scene, op, EMPTY)
    r.set_depth_load_op(A.DEPTH_LOAD)
    st = draw(r, scene, EMPTY, tr)
    assert r.get_depth_load_op() == A.DEPTH_LOAD
    r.set_depth_load_op(A.DEPTH_CLEAR)
    return st


# ---------------------------------------------------------------- 1. two passes equal one
TWO_PASS = ["soup", "soup_rgba8", "soup_scissor", "soup_odd_size", "transparent_layers", "transparent_stack_40",
            "transparent_stack_clipped", "near_clip_wall", "soup_dense_split", "transparent_stack_1300_fallback"]


@pytest.mark.parametrize("instrumented", [True, False], ids=["instrumented", "timed"])
@pytest.mark.parametrize("name", TWO_PASS)
def test_two_passes_equal_one(hip, name, instrumented, monkeypatch):
    for tuning in (0, TUNE_NO_SPLIT):  # with and without the quarter path: tile_load_kernel<.., SPLIT> both ways
        options = ((A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0), (A.OPT_TUNING, tuning))
        if tuning == 0:
            want = run(hip, name, monkeypatch, one_pass, options)  # (the split one pass is the reference for both)
        got = run(hip, name, monkeypatch, two_passes, options)
        assert_same(got, want, f"{name} tuning={tuning}: opaque under CLEAR then transparent under LOAD, against one pass")


@pytest.mark.parametrize("instrumented", [True, False], ids=["instrumented", "timed"])
def test_two_passes_equal_one_on_interleaved_rows(hip, instrumented, monkeypatch):
    options = ((A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0),)
    inter = lambda r: r.set_row_interleave(2, 1)
    want = run(hip, "soup", monkeypatch, one_pass, options, inter)
    got = run(hip, "soup", monkeypatch, two_passes, options, inter)
    owned = LR.owned_mask(160, 96, None, (2, 1))
    assert want["depth"][owned].any() and not want["depth"][~owned].any()  # tile row 1 is drawn, rows 0 and 2 are not
    assert_same(got, want, "soup, rows 2:1")


@pytest.mark.parametrize("instrumented", [True, False], ids=["instrumented", "timed"])
def test_two_passes_equal_one_under_an_odd_scissor(hip, instrumented, monkeypatch):
    options = ((A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0),)
    sci = lambda r: r.set_scissor(*ODD_SCISSOR)
    want = run(hip, "soup", monkeypatch, one_pass, options, sci)
    got = run(hip, "soup", monkeypatch, two_passes, options, sci)
    owned = LR.owned_mask(160, 96, ODD_SCISSOR)
    assert want["depth"][owned].any() and not want["depth"][~owned].any()
    assert_same(got, want, "soup, scissor with an odd origin")


# ---------------------------------------------------------------- 2. the opaque objects split in draw order
OPAQUE_SPLIT = ["hiz_deep_opaque_129", "hiz_deep_opaque_1025", "hiz_deep_opaque_scissor", "hiz_occluder_edges"]


def hiz_rig(lib, sc, instrumented):
    """scenarios.render_hiz with ONE mesh and one material: every layer is an index range of it, so the opaque sort
    (material, mesh, submission index) keeps the layers in submission order in whatever groups they are drawn"""
    rig = SC.Rig(lib, sc.w, sc.h, sc.color_format, background=(0, 0, 0, 1))
    rig.r.set_option(A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0)
    mat = rig.material()
    pos, col, ranges, first = [], [], [], 0
    for layer in sc.layers:
        t = layer.tris
        if not len(t):
            continue
        p = np.empty((len(t) * 3, 3), dtype=f32)
        p[:, 0] = (t[:, :, 0].reshape(-1) * 2.0 / sc.w - 1.0).astype(f32)
        p[:, 1] = (t[:, :, 1].reshape(-1) * 2.0 / sc.h - 1.0).astype(f32)
        p[:, 2] = t[:, :, 2].reshape(-1).astype(f32)
        pos.append(p)
        col += [layer.color] * len(p)
        ranges.append((first, len(p)))
        first += len(p)
    mesh = rig.r.upload_mesh(np.arange(first, dtype=np.uint32), SC.make_vertices(np.concatenate(pos), colors=col))
    objects = SC.objs([SC.render_object(mesh, mat, a, n, extents=(1e6, 1e6, 1e6)) for a, n in ranges])
    if sc.scissor:
        rig.r.set_scissor(*sc.scissor)
    return rig, objects


def split_frame(lib, sc, instrumented, order):
    """order "one": every layer in one pass; "forward": the first half under CLEAR, the second under LOAD; "reversed": the
    second half under CLEAR, the first under LOAD.  -> (frame, depth after the first pass)"""
    rig, objects = hiz_rig(lib, sc, instrumented)
    half = len(objects) // 2
    scene = SC.identity_scene()
    if order == "one":
        rig.draw(scene, objects)
        return rig.finish(), None
    first, second = (objects[:half], objects[half:]) if order == "forward" else (objects[half:], objects[:half])
    rig.draw(scene, first)
    alone = rig.r.read_depth()
    rig.r.set_depth_load_op(A.DEPTH_LOAD)
    rig.r.draw_geometry(scene, second, EMPTY)  # (no clear_color: a deferred clear would land where this pass has no winner)
    return rig.finish(), alone


@pytest.mark.parametrize("instrumented", [True, False], ids=["instrumented", "timed"])
@pytest.mark.parametrize("name", OPAQUE_SPLIT)
def test_opaque_objects_split_in_draw_order(hip, name, instrumented):
    sc = SC.HIZ_GEOMETRY[name]()
    want, _ = split_frame(hip, sc, instrumented, "one")
    forward, d_first = split_frame(hip, sc, instrumented, "forward")
    assert_same(forward, want, f"{name}: first half under CLEAR, second under LOAD (ties go to the later pass)")
    # near half first: the loaded depth hides most of the second pass.  Depth is a maximum whatever the order; colour is
    # decided wherever the halves drawn alone reach different depths (where they tie, the pass order picks the winner)
    backward, d_second = split_frame(hip, sc, instrumented, "reversed")
    assert_same(backward, want, f"{name}: second half under CLEAR, first under LOAD", keys=("depth",))
    decided = bits(d_first) != bits(d_second)
    assert decided.sum() >= 256, "the halves must differ on a good part of the frame"
    assert (bits(d_second) > bits(d_first)).sum() >= 256, "the loaded depth must hide fragments of the second pass"
    assert_same(backward, want, f"{name}: second half under CLEAR, first under LOAD, where no tie decides", keys=("color", "rgba8"),
                where=decided)


# ---------------------------------------------------------------- 3. arbitrary loaded depth through caller-bound tensors
def color_tensor(torch, c0):
    return torch.from_numpy(np.ascontiguousarray(c0).view(np.int16 if c0.dtype == np.uint16 else np.uint8)).cuda()


def random_color(rng, h, w, fmt):
    if fmt == A.COLOR_RGBA8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)


def read_color_tensor(t, c0):
    return t.cpu().numpy().view(c0.dtype).reshape(c0.shape)


def loaded_depth(d, w, h):
    """D0 from the pass's own depth d: zeros, a region of 1.0, a constant plane, exact ties on a checkerboard, and d's two
    neighbours in float order (clamped to [0, 1]: what the header asks of loaded values)"""
    ys, xs = np.mgrid[0:h, 0:w]
    D0 = np.zeros((h, w), f32)
    D0[(xs >= 8) & (xs < 40) & (ys >= 4) & (ys < 30)] = 1.0
    D0[(xs >= 60) & (xs < 100) & (ys >= 10) & (ys < 50)] = 0.55  # (the scene's depths there: 0.52 .. 0.57)
    tie = (xs >= 100) & ((xs + ys) % 2 == 0)
    D0[tie] = d[tie]
    band = (xs < 60) & (ys >= 50)
    up, down = band & ((xs + ys) % 3 == 0), band & ((xs + ys) % 3 == 1)
    D0[up] = np.clip(np.nextafter(d[up], f32(2.0)), 0, 1)
    D0[down] = np.clip(np.nextafter(d[down], f32(-1.0)), 0, 1)
    return D0, {"tie": tie, "up": up, "down": down}


@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8], ids=["rgba16f", "rgba8"])
@pytest.mark.parametrize("w", [160, 150], ids=["w160", "w150_unaligned"])
def test_loaded_depth_from_bound_tensors(hip, w, fmt, monkeypatch):
    torch = pytest.importorskip("torch")
    h = 96
    rng = np.random.default_rng(5 + w + fmt)
    C0 = random_color(rng, h, w, fmt)

    def plan(r, scene, op, tr, draw, extra):
        color = color_tensor(torch, C0)
        depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.bind_targets(color.data_ptr(), depth.data_ptr())
        draw(r, scene, op, EMPTY)  # CLEAR, over C0
        r.sync()
        c, d = read_color_tensor(color, C0), depth.cpu().numpy()
        st_clear = r.get_stats()
        D0, classes = loaded_depth(d, w, h)
        color.copy_(color_tensor(torch, C0))
        depth.copy_(torch.from_numpy(D0).cuda())
        torch.cuda.synchronize()
        r.set_depth_load_op(A.DEPTH_LOAD)
        st = draw(r, scene, op, EMPTY)
        r.sync()
        st_load = r.get_stats()
        r.set_depth_load_op(A.DEPTH_CLEAR)
        extra.update(c=c, d=d, D0=D0, classes=classes, got_c=read_color_tensor(color, C0), got_d=depth.cpu().numpy(),
                     st_clear=st_clear, st_load=st_load)
        r.bind_targets(None, None)
        return st

    # scenarios.SCENARIOS["soup_opaque_only"], at this width and colour format
    out = run(hip, lambda lib: SC.random_soup(lib, w=w, h=h, seed=3, transparent_every=0, n_tris=900, color_format=fmt), monkeypatch, plan)
    c, d, D0, cls = out["c"], out["d"], out["D0"], out["classes"]
    db, lb = bits(d), bits(D0)
    covered = np.any(c != C0, axis=-1)
    assert (covered & cls["tie"]).sum() >= 256 and (covered & cls["up"] & (lb > db)).sum() >= 64 and (covered & cls["down"] & (lb < db)).sum() >= 64
    assert (covered & (D0 == 1.0)).sum() >= 64 and (covered & (D0 == f32(0.55)) & (db > lb)).any() and (covered & (D0 == f32(0.55)) & (db < lb)).any()
    want_d = np.maximum(lb, db)
    bad = bits(out["got_d"]) != want_d
    assert not bad.any(), f"depth: {int(bad.sum())} pixels are not max(loaded, drawn), first at (y, x) = {np.argwhere(bad)[0].tolist()}"
    want_c = np.where((db >= lb)[..., None], c, C0)
    bad = np.any(out["got_c"] != want_c, axis=-1)
    assert not bad.any(), f"colour: {int(bad.sum())} pixels differ, first at (y, x) = {np.argwhere(bad)[0].tolist()}"
    # stats report as for the CLEAR pass of the same objects (instrumented passes drop nothing)
    for f in ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "binned_triangles", "bin_entries"):
        assert getattr(out["st_load"], f) == getattr(out["st_clear"], f), f


def test_transparent_objects_behind_loaded_depth_change_nothing(hip, monkeypatch):
    torch = pytest.importorskip("torch")
    w, h = 160, 96
    x0, y0, x1, y1 = 24, 10, 120, 80
    C0 = random_color(np.random.default_rng(17), h, w, A.COLOR_RGBA16F)

    def plan(r, scene, op, tr, draw, extra):
        color = color_tensor(torch, C0)
        depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.bind_targets(color.data_ptr(), depth.data_ptr())
        draw(r, scene, op, tr)  # the CLEAR render
        r.sync()
        extra["d"] = depth.cpu().numpy()
        extra["c"] = read_color_tensor(color, C0)
        D0 = np.zeros((h, w), f32)
        D0[y0:y1, x0:x1] = 1.0
        color.copy_(color_tensor(torch, C0))
        depth.copy_(torch.from_numpy(D0).cuda())
        torch.cuda.synchronize()
        r.set_depth_load_op(A.DEPTH_LOAD)
        st = draw(r, scene, EMPTY, tr)
        r.sync()
        r.set_depth_load_op(A.DEPTH_CLEAR)
        extra.update(D0=D0, got_c=read_color_tensor(color, C0), got_d=depth.cpu().numpy())
        r.bind_targets(None, None)
        return st

    out = run(hip, "soup", monkeypatch, plan)
    assert out["d"].max() < 1.0, "the soup's fragments stay below depth 1.0"
    assert np.any(out["c"][y0:y1, x0:x1] != C0[y0:y1, x0:x1], axis=-1).sum() >= 1024, "the CLEAR render draws on the rectangle"
    assert np.array_equal(bits(out["got_d"]), bits(out["D0"])), "transparent fragments write no depth"
    assert np.array_equal(out["got_c"][y0:y1, x0:x1], C0[y0:y1, x0:x1]), "behind depth 1.0 nothing is blended"
    outside = np.ones((h, w), bool)
    outside[y0:y1, x0:x1] = False
    assert (np.any(out["got_c"] != C0, axis=-1) & outside).sum() >= 256, "over depth 0.0 the transparent objects are blended"


# ---------------------------------------------------------------- 4. the deferred chain
def deferred(lights=None, ids=False):
    """opaque objects into colour, depth and the G-buffer planes; the lighting pass; the transparent objects under LOAD"""
    def plan(r, scene, op, tr, draw, extra):
        r.enable_attributes(GBUFFER)
        if ids:
            r.enable_ids()
        draw(r, scene, op, EMPTY)
        ambient, sun_dir, sun_color = LR.lighting_of(scene)
        kw = {}
        if lights is not None:
            depth, normal, albedo = r.read_depth(), r.read_attribute(A.ATTR_NORMAL), r.read_attribute(A.ATTR_ALBEDO)
            ref = LR.run_ref(depth, normal, albedo, LR.inv_viewproj(scene.viewproj), ambient, sun_dir, sun_color)
            kw["lights"] = extra["lights"] = lights(ref)
            extra["unlit"] = r.read_color()
        r.light_pass(LR.inv_viewproj(scene.viewproj), ambient, sun_dir, sun_color, **kw)
        before = {"normal": r.read_attribute(A.ATTR_NORMAL), "albedo": r.read_attribute(A.ATTR_ALBEDO), "depth": r.read_depth(),
                  "lit": r.read_color()}
        if ids:
            before["ids"] = r.read_ids()
        r.set_depth_load_op(A.DEPTH_LOAD)
        st = draw(r, scene, EMPTY, tr)
        r.set_depth_load_op(A.DEPTH_CLEAR)
        after = {"normal": r.read_attribute(A.ATTR_NORMAL), "albedo": r.read_attribute(A.ATTR_ALBEDO)}
        if ids:
            after["ids"] = r.read_ids()
        extra.update(before=before, after=after)
        return st
    return plan


@pytest.mark.parametrize("ids", [False, True], ids=["planes", "planes_and_ids"])
@pytest.mark.parametrize("name", ["soup", "transparent_stack_40"])
def test_deferred_chain_equals_the_forward_frame(hip, name, ids, monkeypatch):
    want = run(hip, name, monkeypatch, one_pass)
    got = run(hip, name, monkeypatch, deferred(ids=ids))
    assert_same(got, want, f"{name}: opaque pass, light pass, transparent objects under LOAD, against the forward frame")
    before, after = got["before"], got["after"]
    assert bits(before["albedo"])[..., 3].any(), "the opaque pass has winners"
    for key in after:
        assert np.array_equal(bits(after[key]), bits(before[key])), f"{name}: the LOAD pass changed the {key} target"
    assert np.array_equal(bits(got["depth"]), bits(before["depth"])), f"{name}: transparent objects write no depth"


def test_deferred_chain_with_point_lights(hip, monkeypatch):
    torch = pytest.importorskip("torch")
    from test_lighting_gpu import make_lights
    w, h = 160, 96
    got = run(hip, "soup", monkeypatch, deferred(lights=lambda ref: make_lights(33, ref, seed=23)))
    lit, depth = got["before"]["lit"], got["before"]["depth"]
    assert np.any(lit != got["unlit"], axis=-1).sum() >= 256, "the lights must reach the frame"

    def plan(r, scene, op, tr, draw, extra):  # the lit colour and the depth as a caller's images, then the same LOAD pass
        color = color_tensor(torch, lit)
        d = torch.from_numpy(depth).cuda()
        torch.cuda.synchronize()
        r.bind_targets(color.data_ptr(), d.data_ptr())
        r.set_depth_load_op(A.DEPTH_LOAD)
        st = draw(r, scene, EMPTY, tr)
        r.sync()
        extra.update(got_c=read_color_tensor(color, lit), got_d=d.cpu().numpy())
        r.set_depth_load_op(A.DEPTH_CLEAR)
        r.bind_targets(None, None)
        return st

    want = run(hip, "soup", monkeypatch, plan)
    assert np.any(want["got_c"] != lit, axis=-1).sum() >= 256, "the transparent objects must reach the frame"
    T.assert_images_identical(got["color"], want["got_c"], "the chain's frame against the LOAD pass over the lit colour as a caller's image")
    T.assert_images_identical(got["depth"], want["got_d"], "depth")
    assert w == lit.shape[1] and h == lit.shape[0]


# ---------------------------------------------------------------- 5. replay after a queue overflow
@pytest.mark.parametrize("where", ["clear_pass", "load_pass"])
def test_replayed_after_a_queue_overflow(hip, where, monkeypatch):
    def plan(r, scene, op, tr, draw, extra):
        r.set_option(A.OPT_TUNING, TUNE_NO_POLL)
        if where == "clear_pass":
            r.set_option(A.OPT_QUEUE_CAPS, 64)  # the CLEAR pass overflows: the LOAD pass behind it runs void, both are replayed
        draw(r, scene, op, EMPTY)
        if where == "load_pass":
            r.set_option(A.OPT_QUEUE_CAPS, 64)  # (fences: the CLEAR pass is done) the LOAD pass overflows and is replayed
        r.set_depth_load_op(A.DEPTH_LOAD)
        st = draw(r, scene, EMPTY, tr)
        r.set_depth_load_op(A.DEPTH_CLEAR)
        r.sync()
        extra["replayed"] = r.get_stats().replayed_passes
        return st

    want = run(hip, "soup", monkeypatch, two_passes)
    got = run(hip, "soup", monkeypatch, plan)
    assert want["stats"].replayed_passes == 0 and got["replayed"] > 0
    assert_same(got, want, f"soup, queue overflow in the {where}")


# ---------------------------------------------------------------- 6. refusals and state
def soup_rig(lib, w=160, h=96):
    """a context holding a drawn frame (the atrium's opaque and transparent objects) -> (renderer, scene, opaque, transparent)"""
    r, scene, opaque, transparent = T.setup_sponza(lib, w, h)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    return r, scene, opaque, transparent


STAT_FIELDS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "shaded_fragments", "binned_triangles",
               "bin_entries", "replayed_passes")


def snapshot(r):
    st = r.get_stats()
    return r.read_color(), r.read_depth(), tuple(getattr(st, f) for f in STAT_FIELDS)


def assert_unchanged(r, snap, what):
    now = snapshot(r)
    assert np.array_equal(now[0], snap[0]) and np.array_equal(bits(now[1]), bits(snap[1])) and now[2] == snap[2], what


def test_multiview_and_depth_only_calls_are_refused_under_load(hip):
    torch = pytest.importorskip("torch")
    w, h = 160, 96
    r, scene, opaque, transparent = soup_rig(hip, w, h)
    snap = snapshot(r)
    color = torch.full((2, h, w, 2), 0x3C003C00, dtype=torch.int32, device="cuda")
    depth = torch.full((2, h, w), 0.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lst = r.create_draw_list(opaque, transparent)
    r.set_depth_load_op(A.DEPTH_LOAD)
    calls = {
        "svr_draw_geometry_views": lambda: r.draw_views([scene, scene], color.data_ptr(), depth.data_ptr(), opaque, transparent),
        "svr_draw_list_views": lambda: r.draw_list_views([scene, scene], lst, color.data_ptr(), depth.data_ptr()),
        "svr_draw_depth_views": lambda: r.draw_depth_views([scene, scene], depth.data_ptr(), opaque),
        "svr_draw_list_depth_views": lambda: r.draw_list_depth_views([scene, scene], lst, depth.data_ptr()),
        "svr_draw_depth": lambda: r.draw_depth(scene, opaque),
        "svr_draw_list_depth": lambda: r.draw_list_depth(scene, lst),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.SvrError, match=name + ".*SVR_DEPTH_LOAD") as e:
            call()
        assert e.value.code == -5, name
        assert r.get_depth_load_op() == A.DEPTH_LOAD
        assert_unchanged(r, snap, name)
    r.sync()
    assert torch.all(depth == 0.25).item() and torch.all(color == 0x3C003C00).item(), "the views' targets are untouched"
    r.set_depth_load_op(A.DEPTH_CLEAR)
    for name, call in calls.items():  # the same calls are fine under CLEAR
        call()
    lst.close()
    r.close()


def test_a_bad_op_is_refused(hip):
    r = hip.create(32, 32)
    assert r.get_depth_load_op() == A.DEPTH_CLEAR
    r.set_depth_load_op(A.DEPTH_LOAD)
    for bad in (2, -1, 1 << 20):
        with pytest.raises(pkg.SvrError, match="svr_set_depth_load_op") as e:
            r.set_depth_load_op(bad)
        assert e.value.code == -1
        assert r.get_depth_load_op() == A.DEPTH_LOAD
    r.close()


def test_clear_again_is_a_fresh_context(hip):
    w, h = 160, 96
    want = T.render_sponza(hip, w, h, instrument=True)
    r, scene, opaque, transparent = soup_rig(hip, w, h)
    r.set_depth_load_op(A.DEPTH_LOAD)
    r.draw_geometry(scene, opaque[::2], transparent)
    r.set_depth_load_op(A.DEPTH_CLEAR)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    got = T._finish(r)
    r.close()
    assert_same(got, want, "a CLEAR pass after LOAD passes, against a fresh context")
    for f in STAT_FIELDS:
        assert getattr(got["stats"], f) == getattr(want["stats"], f), f


def test_tex_image_still_clears_under_load(hip):
    w, h = 160, 96
    want = T.render_config2(hip, w, h, instrument=True)
    r, scene, opaque, transparent = soup_rig(hip, w, h)  # depth in the target
    assert r.read_depth().any()
    r.set_depth_load_op(A.DEPTH_LOAD)
    cube = S.cube_mesh()
    mesh = r.upload_mesh(cube.indices, cube.vertices)
    img = r.create_image(S.checkerboard_32(), mipmapped=False)
    smp = r.create_sampler(**S.SAMPLER_NEAREST)
    r.clear_color((1, 1, 1, 1))
    r.draw_tex_image(mesh, 0, cube.indices.size, S.config2_render_matrix(w, h), img, smp)
    got = T._finish(r)
    r.close()
    assert_same(got, want, "svr_draw_tex_image under LOAD, against a fresh context")


@pytest.mark.parametrize("instrumented", [True, False], ids=["instrumented", "timed"])
def test_an_empty_load_pass_changes_nothing(hip, instrumented):
    r, scene, opaque, transparent = soup_rig(hip)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1 if instrumented else 0)
    color, depth = r.read_color(), r.read_depth()
    assert depth.any()
    r.set_depth_load_op(A.DEPTH_LOAD)
    r.draw_geometry(scene, EMPTY, EMPTY)
    assert np.array_equal(r.read_color(), color) and np.array_equal(bits(r.read_depth()), bits(depth))
    r.set_depth_load_op(A.DEPTH_CLEAR)
    r.draw_geometry(scene, EMPTY, EMPTY)  # ... where an empty CLEAR pass clears depth and leaves colour
    assert np.array_equal(r.read_color(), color) and not r.read_depth().any()
    r.close()
