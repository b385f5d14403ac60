"""The object and primitive ID target (include/svr_ids.h) on the MI355X.

There is no ID oracle.  The IDs are checked by isolation against the CPU oracle's depth instead: an object (or one
triangle of it) rendered alone must reach the full frame's depth at every pixel the ID map gives it.  Besides that,
every path that builds draw records (host flatten, device flatten, draw list) and every tile-kernel variant
(instrumented or not, hierarchical depth test on or off) must give the same map, and enabling IDs must change
nothing else.  Every comparison is bit for bit."""
import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu

TUNE_NO_HIZ, TUNE_HIZ = 32, 64  # SVR_OPT_TUNING bits (csrc/svr_device.h)
TUNE_NO_SPLIT = 8  # SVR_OPT_TUNING bit 3: no tile is split, launch_tiles picks the instances without the quarter path
HIP_STATS = ("triangle_count", "drawcall_count", "culled_draws", "rasterized_fragments", "shaded_fragments",
             "binned_triangles", "bin_entries")
# scenarios whose objects are few enough to isolate one by one on the oracle (and with no fragment at depth 0.0)
ISOLATED = ["shading_up", "shared_edge", "fan", "depth_later_nearer", "depth_later_farther", "depth_tie",
            "tex_trilinear", "floor_trilinear", "near_clip_wall", "depth_plane_85", "soup", "soup_opaque_only",
            "soup_scissor", "soup_odd_size", "ragged"]

# scenarios where opaque fragments at depth 0.0 win pixels (ties with the cleared depth go to the fragment)
DEPTH_ZERO_WINS = {"hiz_depth_extremes"}


def _objects(a):
    if a is None:
        return np.zeros(0, A.RENDER_OBJECT_DTYPE)
    return np.ascontiguousarray(a, dtype=A.RENDER_OBJECT_DTYPE).reshape(-1)


def run(lib, name, mp, ids=True, path="host", options=(), opaque_filter=None, drop_transparent=False):
    """Scenario `name` with its draw_geometry call rerouted: IDs on or off, the host flatten, the device flatten or a
    draw list, extra options, and the opaque list filtered (opaque_filter(list) -> list).  Returns T._finish's frame,
    plus "ids" when they were on."""
    orig_draw, orig_finish = A.Renderer.draw_geometry, T._finish

    def draw(self, scene, opaque, transparent=None):
        op, tr = _objects(opaque), _objects(transparent)
        if opaque_filter is not None:
            op = _objects(opaque_filter(op))
        if drop_transparent:
            tr = _objects(None)
        for k, v in options:
            self.set_option(k, v)
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
        if ids:
            out["ids"] = r.read_ids()
        return out

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        m.setattr(T, "_finish", finish)
        return SC.SCENARIOS[name](lib)


def assert_frames_same(a, b, what, stats=HIP_STATS):
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(a[key], b[key], f"{what} {key}")
    for f in stats:
        assert getattr(a["stats"], f) == getattr(b["stats"], f), f"{what}: {f}"


def assert_ids_same(a, b, what):
    bad = np.any(a != b, axis=-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[0]}"


def assert_ids_match_depth(ids, depth, what):
    """a pixel has an ID exactly where an opaque fragment wrote depth (test scenes have no fragment at depth 0.0)"""
    has_id, has_depth = ids[..., 0] != 0, depth != 0.0
    assert np.array_equal(has_id, has_depth), f"{what}: {int((has_id != has_depth).sum())} pixels disagree"
    assert not np.any((ids[..., 0] == 0) & (ids[..., 1] != 0)), f"{what}: primitive without object"


# ---------------------------------------------------------------- 1. nothing else changes; 2. one map on every path
@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_ids_change_nothing_and_agree_on_every_path(hip, name, monkeypatch):
    if name == "soup_very_dense_split":  # over the draw list's object cap: the host and device flatten only
        paths = ("host", "device")
    else:
        paths = ("host", "device", "list")
    want = run(hip, name, monkeypatch, ids=False)
    first = None
    for path in paths:
        got = run(hip, name, monkeypatch, path=path)
        assert_frames_same(got, want, f"{name} {path}")
        if first is None:
            first = got["ids"]
            if name in DEPTH_ZERO_WINS:  # a fragment at depth 0.0 wins there: an ID wherever depth is not 0.0
                assert np.all(first[..., 0][got["depth"] != 0.0] != 0), name
            else:
                assert_ids_match_depth(first, got["depth"], name)
        assert_ids_same(got["ids"], first, f"{name} {path}")
    for opts in (((A.OPT_COUNT_FRAGMENTS, 0),), ((A.OPT_TUNING, TUNE_NO_HIZ),), ((A.OPT_TUNING, TUNE_HIZ),),
                 ((A.OPT_COUNT_FRAGMENTS, 0), (A.OPT_TUNING, TUNE_HIZ)),
                 ((A.OPT_TUNING, TUNE_NO_SPLIT),), ((A.OPT_COUNT_FRAGMENTS, 0), (A.OPT_TUNING, TUNE_NO_SPLIT))):
        got = run(hip, name, monkeypatch, options=opts)
        assert_ids_same(got["ids"], first, f"{name} {opts}")
        if opts[-1] == (A.OPT_TUNING, TUNE_NO_SPLIT):  # the instances without the quarter path: the whole frame, not only the IDs
            assert_frames_same(got, want, f"{name} {opts}", stats=())


def _sponza_frame(hip, w, h, instanced, path="host", ids=True, options=()):
    kw = dict(camera=S.config5_camera(), instances=S.config5_instances()) if instanced else {}
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=64, **kw)
    for k, v in options:
        r.set_option(k, v)
    if ids:
        r.enable_ids()
    r.clear_color((1, 1, 1, 1))
    if path == "list":
        lst = r.create_draw_list(opaque, transparent)
        r.draw_list(scene, lst)
        lst.close()
    else:
        r.set_option(A.OPT_DEVICE_FLATTEN, 1 if path == "device" else 2)
        r.draw_geometry(scene, opaque, transparent)
    out = {"color": r.read_color(), "depth": r.read_depth(), "stats": r.get_stats()}
    if ids:
        out["ids"] = r.read_ids()
    r.close()
    return out


FULL = {"config2_1920x1080": (1920, 1080, False), "config3_3840x2160": (3840, 2160, False),
        "config4_x16_7680x4320": (7680, 4320, True)}


@pytest.mark.parametrize("name", list(FULL))
def test_full_frames(hip, name):
    """Uninstrumented passes at full size, where the hierarchical depth test really drops triangles."""
    w, h, inst = FULL[name]
    want = _sponza_frame(hip, w, h, inst, ids=False)
    base = _sponza_frame(hip, w, h, inst)
    for key in ("color", "depth"):
        T.assert_images_identical(base[key], want[key], f"{name} {key}")
    for f in ("triangle_count", "drawcall_count", "culled_draws"):
        assert getattr(base["stats"], f) == getattr(want["stats"], f), f
    assert_ids_match_depth(base["ids"], base["depth"], name)
    assert (base["ids"][..., 0] != 0).mean() > 0.5
    variants = [("device", ()), ("list", ()), ("host", ((A.OPT_TUNING, TUNE_NO_HIZ),))]
    if not inst:
        variants.append(("host", ((A.OPT_COUNT_FRAGMENTS, 1),)))
    for path, opts in variants:
        got = _sponza_frame(hip, w, h, inst, path=path, options=opts)
        T.assert_images_identical(got["depth"], want["depth"], f"{name} {path} {opts} depth")
        assert_ids_same(got["ids"], base["ids"], f"{name} {path} {opts}")


# ---------------------------------------------------------------- 3. truth by isolation on the oracle
@pytest.mark.parametrize("name", ISOLATED)
def test_ids_against_the_oracle_by_isolation(hip, oracle, name, monkeypatch):
    got = run(hip, name, monkeypatch)
    ids = got["ids"]
    full = run(oracle, name, monkeypatch, ids=False)
    depth = full["depth"]
    T.assert_images_identical(got["depth"], depth, name + " depth")
    opaque_only = run(oracle, name, monkeypatch, ids=False, drop_transparent=True)["depth"]
    assert np.array_equal(ids[..., 0] == 0, opaque_only == 0.0), name
    objects = sorted(set(int(o) for o in np.unique(ids[..., 0])) - {0})
    rng = np.random.default_rng(1234)
    if len(objects) > 24:
        objects = sorted(rng.choice(objects, 24, replace=False).tolist())
    for o in objects:
        alone = run(oracle, name, monkeypatch, ids=False, drop_transparent=True, opaque_filter=lambda op, o=o: op[o - 1:o])["depth"]
        mine = ids[..., 0] == o
        assert np.array_equal(alone[mine], depth[mine]), f"{name}: object {o} does not reach the depth where it is named"
    ys, xs = np.nonzero(ids[..., 0])
    pick = rng.choice(len(ys), min(24, len(ys)), replace=False) if len(ys) else []
    for i in pick:
        y, x = int(ys[i]), int(xs[i])
        o, p = int(ids[y, x, 0]), int(ids[y, x, 1])

        def one_triangle(op, o=o, p=p):
            t = op[o - 1:o].copy()
            t["first_index"] = t["first_index"] + 3 * p
            t["index_count"] = 3
            return t
        alone = run(oracle, name, monkeypatch, ids=False, drop_transparent=True, opaque_filter=one_triangle)["depth"]
        assert alone[y, x] == depth[y, x], f"{name}: pixel ({x}, {y}) names triangle {p} of object {o}"


# ---------------------------------------------------------------- 4.-6. ties, transparent objects, clipping
def test_depth_tie_names_the_later_object(hip, monkeypatch):
    # two coplanar quads over the whole target, same material and sort key: draw order is submission order, and the
    # tie rule (max over (depth, key)) gives every pixel to the second
    ids = run(hip, "depth_tie", monkeypatch)["ids"]
    assert np.all(ids[..., 0] == 2)
    assert set(np.unique(ids[..., 1]).tolist()) == {0, 1}  # the quad's two triangles


def test_transparent_objects_leave_the_ids(hip, monkeypatch):
    for name in ("soup", "soup_rgba8", "transparent_layers"):
        with_tr = run(hip, name, monkeypatch)["ids"]
        without = run(hip, name, monkeypatch, drop_transparent=True)["ids"]
        assert_ids_same(with_tr, without, name)


def test_clipped_triangles_report_their_parent(hip, monkeypatch):
    ids = run(hip, "near_clip_wall", monkeypatch)["ids"]
    assert np.all(ids[..., 0] <= 1) and set(np.unique(ids[..., 1]).tolist()) <= {0, 1}
    assert (ids[..., 0] == 1).any()
    # the transparent stack crosses the near plane too, but transparent objects write no ID
    ids = run(hip, "transparent_stack_clipped", monkeypatch)["ids"]
    assert not ids.any()


# ---------------------------------------------------------------- 7.-9. ownership, replay, binding, draw lists
SENTINEL = 0x5A5A5A5A


def _torch_target(w, h):
    torch = pytest.importorskip("torch")
    t = torch.full((h, w, 2), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return torch, t


def _sponza_small(hip, w=256, h=144):
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    return r, scene, opaque, transparent


def test_scissor_and_row_interleave_write_owned_pixels_only(hip):
    w, h = 256, 144
    r, scene, opaque, transparent = _sponza_small(hip, w, h)
    r.enable_ids()
    r.draw_geometry(scene, opaque, transparent)
    full = r.read_ids()
    torch, t = _torch_target(w, h)
    r.bind_id_target(t.data_ptr())
    assert r.get_id_target() == t.data_ptr()
    x0, y0, sw, sh = 37, 21, 101, 77
    r.set_scissor(x0, y0, sw, sh)
    r.draw_geometry(scene, opaque, transparent)
    got = r.read_ids()
    mask = np.zeros((h, w), bool)
    mask[y0:y0 + sh, x0:x0 + sw] = True
    assert_ids_same(got[mask], full[mask], "scissor")
    assert np.all(got[~mask] == SENTINEL)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), got)
    # interleaved rows: of the 32-row tile rows, those with index % 3 == 1
    t.fill_(SENTINEL)
    torch.cuda.synchronize()
    r.set_scissor(0, 0, w, h)
    r.set_row_interleave(3, 1)
    r.draw_geometry(scene, opaque, transparent)
    got = r.read_ids()
    rows = (np.arange(h) // 32) % 3 == 1
    assert_ids_same(got[rows], full[rows], "interleave")
    assert np.all(got[~rows] == SENTINEL)
    # passes that are not geometry passes leave the target alone
    r.set_row_interleave(1, 0)
    r.clear_color((0.5, 0.5, 0.5, 1))
    r.draw_background(0, A.GRADIENT_DEFAULT)
    r.draw_colored_triangle()
    assert_ids_same(r.read_ids(), got, "other passes")
    r.bind_id_target(None)
    assert_ids_same(r.read_ids(), full, "back to the context's plane")
    r.enable_ids(False)
    assert r.get_id_target() is None
    with pytest.raises(A.SvrError):
        r.read_ids()
    r.close()


def test_replay_writes_the_target_of_its_pass(hip):
    w, h = 256, 144
    r, scene, opaque, transparent = _sponza_small(hip, w, h)
    r.enable_ids()
    r.draw_geometry(scene, opaque, transparent)
    want = r.read_ids()
    r.close()
    r, scene, opaque, transparent = _sponza_small(hip, w, h)
    r.set_option(A.OPT_QUEUE_CAPS, 64)
    r.set_option(A.OPT_TUNING, 16)  # TUNE_NO_POLL: the overflow is found at the fence, after the unbind below
    torch, t = _torch_target(w, h)
    r.bind_id_target(t.data_ptr())
    r.draw_geometry(scene, opaque, transparent)
    r.bind_id_target(None)  # no ID target from here on: the pass and its replay still write t
    r.sync()
    assert r.get_stats().replayed_passes > 0
    assert r.get_id_target() is None
    assert_ids_same(t.cpu().numpy().view(np.uint32), want, "replayed pass")
    with pytest.raises(A.SvrError, match="no ID target"):
        r.pick(0, 0)
    r.close()


def test_draw_list_update_and_pick(hip):
    w, h = 256, 144
    r, scene, opaque, transparent = _sponza_small(hip, w, h)
    r.enable_ids()
    lst = r.create_draw_list(opaque, transparent)
    r.draw_list(scene, lst)
    before = r.read_ids()
    # the biggest object on screen moves away: the IDs follow the new objects, as the host path gives them
    objs, counts = np.unique(before[..., 0], return_counts=True)
    big = int(objs[1:][np.argmax(counts[1:])])
    moved = opaque.copy()
    far = np.eye(4, dtype=np.float32).reshape(16)
    far[13] = -1.0e4  # column-major: a translation far below the camera (culled)
    moved["transform"][big - 1] = far
    lst.update(big - 1, moved[big - 1:big])
    r.draw_list(scene, lst)
    after = r.read_ids()
    r.draw_geometry(scene, moved, transparent)
    assert_ids_same(after, r.read_ids(), "updated list")
    assert not np.array_equal(after, before) and not (after[..., 0] == big).any()
    rng = np.random.default_rng(7)
    for _ in range(64):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        p = r.pick(x, y)
        o, q = int(after[y, x, 0]), int(after[y, x, 1])
        assert p == (None if o == 0 else (o, q))
    for x, y in ((w, 0), (0, h)):
        with pytest.raises(A.SvrError):
            r.pick(x, y)
    lst.close()
    r.close()
