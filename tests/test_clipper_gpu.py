"""The clipper of the binning launch (csrc/k_bin.hip clip_and_bin) where the per-case tests of family D cannot reach.

Every instance sees the same pieces: each case of tests/raster_cases.py family D (the clip volume and the guard band) is
drawn plain, uninstrumented, without split tiles, with an ID target, depth-only, as a two-layer multiview pass with one
camera in both layers, and from a retained draw list.  Colour and depth are the plain pass's bit for bit, the plain pass
is the oracle's, and the ID plane names, at every covered pixel farther than tau from the ideal boundary, the parent
triangle that tests/raster_ref.py names - in the pairs that share a cut edge the right one of the two.

Lanes and strides: one pass of N small triangles that each cross the near or the far plane, for N around the clipper's
lane count, around a wave's worth of lanes, and beyond clip_blocks * CLIP_LANES, where its grid-stride loop takes a second
step.  Polygons of 3 to 7 vertices in seeded order, so that the lanes of a wave fan to different lengths and some finish
degenerate; mixed depths, every fifth triangle transparent.  Frame and stats are the oracle's bit for bit, with and
without an ID target.  Then the same pass from queues of 64 entries: clip queue and piece records overflow, the pass is
replayed, the frame is the same."""
import re

import numpy as np
import pytest

import raster_cases as RC
import raster_ref as RR
import scenarios as SC
import svr_testlib as T
from test_timed_paths_gpu import COUNTS, INSTR_COUNTS, TUNE_NO_SPLIT

A = SC.A
f32 = np.float32
gpu = pytest.mark.gpu
TUNE_NO_POLL = 16  # SVR_OPT_TUNING bit (csrc/svr_device.h; test_the_constants_are_the_ones_the_sources_use)


# ---------------------------------------------------------------- every instance sees the same pieces
def _frame(r):
    return {"color": r.read_color(), "depth": r.read_depth()}


def _same(got, want, what, keys=("color", "depth")):
    for key in keys:
        T.assert_images_identical(got[key], want[key], f"{what} {key}")


def _check_ids(ids, owners, what):
    """owners: [(reference of one triangle's pass, its primitive index)]"""
    sure_out = np.ones(ids.shape[:2], bool)
    for ref, prim in owners:
        sure = ref.covered & ~ref.offered
        assert np.all(ids[sure, 0] == 1) and np.all(ids[sure, 1] == prim), f"{what}: the ID plane does not name primitive {prim} where it covers"
        sure_out &= ~ref.covered & ~ref.offered
    assert not ids[sure_out].any(), f"{what}: an ID where nothing is drawn"


@gpu
@pytest.mark.parametrize("group", RC.D_GROUPS)
def test_every_instance_sees_the_same_pieces(hip, oracle, group):
    pytest.importorskip("torch")  # the layered targets are torch tensors; nothing else may make this test skip
    import test_views_gpu as views
    cases = [c for c in RC.cases("D") if c.group == group]
    w, h = cases[0].width, cases[0].height
    plain, with_ids, ora = RC.Rig(hip, w, h), RC.Rig(hip, w, h), RC.Rig(oracle, w, h)
    with_ids.r.enable_ids()
    try:
        for k, case in enumerate(cases):
            lead = 1 + k % 3
            mesh, ro, scene = plain.prepare(case, lead=lead)
            r = plain.r

            def draw(instrumented=1, tuning=0, how=None):
                r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
                r.set_option(A.OPT_TUNING, tuning)
                r.clear_color((0.0, 0.0, 0.0, 0.0))
                (how or (lambda: r.draw_geometry(scene, ro)))()
                return _frame(r)

            want = draw()
            mo, roo, so = ora.prepare(case, lead=lead)
            ora.r.clear_color((0.0, 0.0, 0.0, 0.0))
            ora.r.draw_geometry(so, roo)
            _same(want, _frame(ora.r), f"{case.name}: the plain pass against the oracle's")
            ora.r.destroy_mesh(mo)
            for instrumented, tuning in ((0, 0), (0, TUNE_NO_SPLIT), (1, TUNE_NO_SPLIT)):
                _same(draw(instrumented, tuning), want, f"{case.name}: instrumented {instrumented}, tuning {tuning}")
            lst = r.create_draw_list(ro)
            _same(draw(how=lambda: r.draw_list(scene, lst)), want, f"{case.name}: from a retained draw list")
            _same(draw(0, 0, how=lambda: r.draw_depth(scene, ro)), want, f"{case.name}: depth-only", keys=("depth",))
            _same(draw(0, 0, how=lambda: r.draw_list_depth(scene, lst)), want, f"{case.name}: depth-only from a draw list", keys=("depth",))
            lst.close()
            for instrumented in (1, 0):
                r.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
                got, _ = views._views(r, [scene, scene], ro, None, None, clear=(0.0, 0.0, 0.0, 0.0))
                for layer in (0, 1):
                    _same({key: v[layer] for key, v in got.items()}, want, f"{case.name}: multiview layer {layer}, instrumented {instrumented}")
            color, depth, _ = views._layers(r, 2)
            r.draw_depth_views([scene, scene], depth.data_ptr(), ro)
            got = views._read(r, color, depth, None)
            for layer in (0, 1):
                _same({"depth": got["depth"][layer]}, want, f"{case.name}: depth-only multiview layer {layer}", keys=("depth",))
            r.destroy_mesh(mesh)
            # with an ID target: the same frame, and the parent the reference names
            ref = RC.reference(case)
            mesh, ro, scene = with_ids.prepare(case, lead=lead)
            ri = with_ids.r
            for instrumented in (1, 0):
                ri.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
                ri.clear_color((0.0, 0.0, 0.0, 0.0))
                ri.draw_geometry(scene, ro)
                _same(_frame(ri), want, f"{case.name}: with an ID target, instrumented {instrumented}")
                _check_ids(ri.read_ids(), [(ref, lead)], f"{case.name}, instrumented {instrumented}")
            ri.draw_depth(scene, ro)
            _same(_frame(ri), want, f"{case.name}: depth-only with an ID target", keys=("depth",))
            _check_ids(ri.read_ids(), [(ref, lead)], f"{case.name}, depth-only")
            idt = views._layers(ri, 2, ids=True)
            ri.draw_views([scene, scene], idt[0].data_ptr(), idt[1].data_ptr(), ro, None, ids_ptr=idt[2].data_ptr(), clear_rgba=(0.0, 0.0, 0.0, 0.0))
            got = views._read(ri, *idt)
            for layer in (0, 1):
                _same({key: got[key][layer] for key in ("color", "depth")}, want, f"{case.name}: multiview with IDs, layer {layer}")
                _check_ids(got["ids"][layer], [(ref, lead)], f"{case.name}, multiview layer {layer}")
            ri.destroy_mesh(mesh)
            if case.pair:  # both halves in one pass: each pixel names the half that covers it
                first = cases[k - 1]
                mesh, ro, scene = with_ids.prepare(case, tris=first.tris + case.tris, lead=lead)
                ri.clear_color((0.0, 0.0, 0.0, 0.0))
                ri.draw_geometry(scene, ro)
                _check_ids(ri.read_ids(), [(RC.reference(first), lead), (ref, lead + 1)], f"{first.name} + {case.name}")
                ri.destroy_mesh(mesh)
    finally:
        for rig in (plain, with_ids, ora):
            rig.close()


# ---------------------------------------------------------------- lanes and strides
def clip_constants():
    """(clip_blocks, CLIP_LANES) as csrc/k_bin.hip has them"""
    with open(f"{T.ROOT}/simple-vk-renderer_amd/csrc/k_bin.hip") as f:
        src = f.read()
    lanes = re.search(r"constexpr uint32_t CLIP_LANES\s*=\s*(\d+);", src)
    blocks = re.search(r"\bclip_blocks\s*=\s*(\d+)\s*;", src)
    assert lanes and blocks, "k_bin.hip no longer states CLIP_LANES and clip_blocks as this test reads them"
    return int(blocks.group(1)), int(lanes.group(1))


W, H = 96, 64
_SOUP = {}


def soup(n):
    """The first n of a seeded sequence of small triangles in the identity scene (clip = position, w = 1), each crossing
    z = w = 1 or z = 0: (positions (n, 3, 3), colours (n, 4), whether each surely yields a piece: the ideal rule covers a
    pixel centre well inside its band)."""
    total = lane_counts()[-1]
    if "all" not in _SOUP:
        rng = np.random.default_rng(8807)
        pos, col, sure = np.zeros((total, 3, 3), f32), np.zeros((total, 4), f32), np.zeros(total, bool)
        near, far, inside = (lambda: rng.uniform(1.05, 1.6)), (lambda: rng.uniform(-0.6, -0.05)), (lambda: rng.uniform(0.1, 0.9))
        for i in range(total):
            kind = int(rng.integers(0, 6))
            c = rng.uniform((4.0, 4.0), (W - 4.0, H - 4.0))
            if kind == 4:  # over the target's border or corner as well: 6 and 7 vertices
                c = np.array([rng.choice([0.0, W]), rng.choice([0.0, H, rng.uniform(8.0, H - 8.0)])])
            ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
            xy = c + rng.uniform(3.0, 9.0) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
            z = {0: [near(), inside(), inside()],            # 4 vertices
                 1: [near(), near(), inside()],              # 3
                 2: [far(), inside(), inside()],             # 4
                 3: [near(), far(), inside()],               # 5
                 4: [near(), far(), inside()],               # up to 7
                 5: [1.0, near(), near()] if rng.integers(0, 2) else [0.0, far(), far()]}[kind]  # touches a plane: degenerate
            o = rng.permutation(3)
            pos[i, :, 0], pos[i, :, 1], pos[i, :, 2] = xy[:, 0] * 2.0 / W - 1.0, xy[:, 1] * 2.0 / H - 1.0, np.array(z)[o]
            col[i] = (*rng.uniform(0.1, 1.0, 3), 0.5 if i % 5 == 4 else 1.0)
            clip = np.concatenate([pos[i], np.ones((3, 1), f32)], axis=1)
            assert RR.routed_to_clipper(clip, W, H), "every triangle of the soup goes through the clipper"
            outside = np.stack([clip[:, 2] > clip[:, 3], clip[:, 2] < 0] + [s * clip[:, a] > clip[:, 3] for a in (0, 1) for s in (1, -1)])
            assert not outside.all(axis=1).any(), "no plane has all three vertices outside: the triangle is queued, not rejected"
            t = RR.ClippedTri(clip, np.zeros((3, 2), f32), W, H, bounds=False)
            sure[i] = not t.empty and bool((t.signed_distance() > 0.01).any())  # (0.01 px: beyond any tau of this scene)
        _SOUP["all"] = (pos, col, sure)
    pos, col, sure = _SOUP["all"]
    return pos[:n], col[:n], sure[:n]


def draw_soup(lib, n, ids=False, options=()):
    pos, col, _ = soup(n)
    rig = SC.Rig(lib, W, H, background=(0.1, 0.1, 0.1, 1))
    if ids:
        rig.r.enable_ids()
    for opt, value in options:
        rig.r.set_option(opt, value)
    lists = []
    for transparent in (False, True):
        sel = np.nonzero((np.arange(n) % 5 == 4) == transparent)[0]
        if len(sel):
            verts = SC.make_vertices(pos[sel].reshape(-1, 3), colors=np.repeat(col[sel], 3, axis=0))
            mesh = rig.r.upload_mesh(np.arange(len(verts), dtype=np.uint32), verts)
            lists.append([SC.render_object(mesh, rig.material(transparent=transparent), 0, len(verts), extents=RC.BIG)])
        else:
            lists.append([])
    rig.draw(SC.identity_scene(), lists[0], lists[1])
    out = rig.finish() if not ids else None
    if ids:
        out = T._finish(rig.r)
        out["ids"] = rig.r.read_ids()
        rig.r.close()
    return out


def lane_counts():
    blocks, lanes = clip_constants()
    s = blocks * lanes
    return [1, 7, 8, 9, 63, 64, 65, s, s + 1, s + 9]


def test_the_constants_are_the_ones_the_sources_use():
    """(no GPU) S = clip_blocks * CLIP_LANES is the stride only while clip_and_bin's loop, its LDS and the launch are
    written in these two names; the late-found overflow needs the TUNE_NO_POLL bit of svr_device.h"""
    with open(f"{T.ROOT}/simple-vk-renderer_amd/csrc/k_bin.hip") as f:
        src = f.read()
    squeeze = re.sub(r"\s+", "", src)
    for text in ("for(uint32_tq0=block*CLIP_LANES;q0<n;q0+=n_blocks*CLIP_LANES)",      # the grid-stride loop
                 "VOutpoly[CLIP_LANES][12];", "VOuttmp[CLIP_LANES][12];", "TriGeomgeom[CLIP_LANES];",  # a lane's LDS
                 "constboolworker=lane<CLIP_LANES&&q<n;",
                 "clip_and_bin<IDS,MV>(P,s_clip,blockIdx.x-big_blocks,clip_blocks);"):    # the launch's count is the loop's
        assert text in squeeze, f"k_bin.hip no longer has `{text}`: the lane counts of this file may not reach the second step"
    assert len(re.findall(r"\bclip_blocks\s*=\s*\d+", src)) == 1, "one launch, one clip_blocks"
    with open(f"{T.ROOT}/simple-vk-renderer_amd/csrc/svr_device.h") as f:
        m = re.search(r"constexpr uint32_t TUNE_NO_POLL\s*=\s*(\d+)u", f.read())
    assert m and int(m.group(1)) == TUNE_NO_POLL


@gpu
@pytest.mark.parametrize("index", range(10))
def test_lanes_and_strides(hip, oracle, index):
    n = lane_counts()[index]
    want, got = draw_soup(oracle, n), draw_soup(hip, n)
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(got[key], want[key], f"{n} clipped triangles: {key}")
    for f in INSTR_COUNTS:
        assert getattr(got["stats"], f) == getattr(want["stats"], f), f"{n} clipped triangles: {f}"
    # That the clipper took all n: no counter reports its queue.  What shows it is the equality above - binned_triangles
    # and rasterized_fragments are the oracle's, and with every triangle the clipper's (soup asserts that each is routed
    # to it and that no plane has all three vertices outside, which is all the setup kernel asks before it queues one)
    # every binned triangle is a piece of its making: a queue entry left out, a whole stride step say, takes its pieces
    # and fragments out of both counts and its pixels out of the frame.  The counters are also held from below by the
    # triangles that surely yield a piece, and beyond S some of those must lie in the loop's second step.
    sure = soup(n)[2]
    assert got["stats"].triangle_count == n and got["stats"].binned_triangles >= int(sure.sum())
    assert n < 63 or int(sure.sum()) >= n // 2, "the soup is mostly empty"
    s = lane_counts()[7]
    assert n <= s or sure[s:].any(), "no triangle of the second stride step is sure to be seen"
    assert got["stats"].replayed_passes == 0
    with_ids = draw_soup(hip, n, ids=True)
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(with_ids[key], got[key], f"{n} clipped triangles with an ID target: {key}")
    for f in INSTR_COUNTS:
        assert getattr(with_ids["stats"], f) == getattr(got["stats"], f), f"{n} clipped triangles with an ID target: {f}"
    covered = with_ids["depth"] != 0.0
    assert np.all(with_ids["ids"][covered, 0] == 1) and with_ids["ids"][..., 0].max() <= 1, "the opaque object's ID where its pieces wrote depth"
    plain = draw_soup(hip, n, options=((A.OPT_COUNT_FRAGMENTS, 0),))
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(plain[key], want[key], f"{n} clipped triangles, uninstrumented: {key}")
    for f in COUNTS:
        assert getattr(plain["stats"], f) == getattr(want["stats"], f), f"{n} clipped triangles, uninstrumented: {f}"


@gpu
def test_overflowing_clip_queue_and_piece_records(hip):
    n = lane_counts()[-1]
    want = draw_soup(hip, n)
    got = draw_soup(hip, n, options=((A.OPT_QUEUE_CAPS, 64), (A.OPT_TUNING, TUNE_NO_POLL)))
    assert want["stats"].replayed_passes == 0 and got["stats"].replayed_passes > 0
    for key in ("color", "depth", "rgba8"):
        T.assert_images_identical(got[key], want[key], f"{n} clipped triangles from queues of 64: {key}")
    for f in INSTR_COUNTS:
        assert getattr(got["stats"], f) == getattr(want["stats"], f), f"{n} clipped triangles from queues of 64: {f}"
