"""Occlusion culling (include/svr_occlusion.h) on the MI355X.

The pyramid against numpy bit for bit; passes that cull against a pyramid that meets the header's condition (built from
the same pass's depth, "last", or from a depth-only pass of a subset of the opaque objects, "prepass") against the same
pass without culling, bit for bit, on the edge-case scenarios, the atrium and the full-size frames (also against the
oracle's digests); adversarial scenes; both ends of the pyramid; every culled chunk checked in float64; the culled share
at configs[4] x16; stream order with replays and rebuilds; the multiview refusal."""
import importlib.util
import json
import os

import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

_spec = importlib.util.spec_from_file_location("make_full_frames", os.path.join(T.GOLDEN_DIR, "make_full_frames.py"))
MF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MF)

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SAME = ("triangle_count", "drawcall_count", "culled_draws", "shaded_fragments")  # unchanged by culling
ALL = SAME + ("rasterized_fragments", "binned_triangles", "bin_entries")
# configs[4] x16 at 7680x4320, "last": the culled share of triangles measured 0.961; the floor is about half
CULLED_SHARE_FLOOR = 0.48


# ---------------------------------------------------------------- the pyramid in numpy
def np_pyramid(depth):
    """levels 1 .. of the uint32 bit patterns of depth [H, W]: 2x2 minima, the frame's outside as 0xffffffff"""
    cur = np.ascontiguousarray(depth).view(np.uint32)
    out = []
    while True:
        h, w = cur.shape
        pad = np.full((h + (h & 1), w + (w & 1)), 0xffffffff, dtype=np.uint32)
        pad[:h, :w] = cur
        cur = pad.reshape(pad.shape[0] // 2, 2, pad.shape[1] // 2, 2).min(axis=(1, 3))
        out.append(cur)
        if cur.shape == (1, 1):
            return out


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _check_pyramid(r, pyr, depth, what):
    want = np_pyramid(depth)
    assert r.pyramid_levels(pyr) == len(want), what
    for l, lv in enumerate(want, start=1):
        got = r.read_depth_pyramid(pyr, l)
        assert got.shape == lv.shape, f"{what} level {l}"
        if not np.array_equal(got, lv):
            bad = np.argwhere(got != lv)[:5]
            raise AssertionError(f"{what} level {l}: {int((got != lv).sum())} texels differ, first at {bad.tolist()}")


@pytest.mark.parametrize("size", [(1, 1), (33, 17), (160, 90), (1920, 1080), (3840, 2160), (7680, 4320)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_equals_numpy(hip, size):
    w, h = size
    r = hip.create(w, h)
    pyr = r.create_depth_pyramid()
    rng = np.random.default_rng(w * 7 + h)
    sources = {"zeros": np.zeros((h, w), np.float32), "ones": np.ones((h, w), np.float32),
               "denormals": rng.integers(1, 0x800000, (h, w), dtype=np.uint32).view(np.float32),
               "random_bits": rng.integers(0, 2**32, (h, w), dtype=np.uint32).view(np.float32),
               "random": rng.random((h, w), dtype=np.float32)}
    for name, src in sources.items():
        buf = _dev(src)
        r.build_depth_pyramid(pyr, buf.data_ptr())
        _check_pyramid(r, pyr, src, f"{w}x{h} {name}")
        del buf
    r.destroy_depth_pyramid(pyr)
    r.close()


def test_pyramid_of_the_context_depth_after_a_pass(hip):
    r, scene, opaque, transparent = T.setup_sponza(hip, 160, 90, lod=8, tex_size=64)
    pyr = r.create_depth_pyramid()
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    r.build_depth_pyramid(pyr)  # NULL: the context's depth target, unfenced behind the pass
    depth = r.read_depth()
    assert (depth > 0).any()
    _check_pyramid(r, pyr, depth, "context depth")
    r.close()


# ---------------------------------------------------------------- passes with and without culling
def _targets(r, ids, seed=5):
    h, w = r.height, r.width
    px = 8 if r.color_format == A.COLOR_RGBA16F else 4
    rng = np.random.default_rng(seed)
    color = torch.from_numpy(rng.integers(0, 256, (h, w, px), dtype=np.uint8)).cuda()
    depth = torch.from_numpy(rng.random((h, w), dtype=np.float32)).cuda()
    idt = torch.full((h, w, 2), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if ids else None
    torch.cuda.synchronize()
    return color, depth, idt


def _pass(r, draw, ids=True, seed=5):
    """fresh targets bound, draw() run, fenced: the targets after, the stats and the occlusion stats"""
    color, depth, idt = _targets(r, ids, seed)
    r.bind_targets(color.data_ptr(), depth.data_ptr())
    r.bind_id_target(idt.data_ptr() if ids else None)
    draw()
    st = r.get_stats()
    ost = r.occlusion_stats()
    torch.cuda.synchronize()
    out = {"color": color.cpu().numpy(), "depth": depth.cpu().numpy()}
    if ids:
        out["ids"] = idt.cpu().numpy().view(np.uint32)
    r.bind_targets(None, None)
    r.bind_id_target(None)
    return out, st, ost


def _same(got, want, what, gst=None, wst=None, fields=SAME):
    for k in want:
        T.assert_images_identical(got[k], want[k], f"{what} {k}")
    if gst is not None:
        for f in fields:
            assert getattr(gst, f) == getattr(wst, f), f"{what}: {f} {getattr(gst, f)} != {getattr(wst, f)}"


def _drawer(r, scene, opaque, transparent, path):
    if path == "list":
        lst = r.create_draw_list(opaque, transparent)
        return (lambda: r.draw_list(scene, lst)), lst
    if path == "depth":
        return (lambda: r.draw_depth(scene, opaque)), None
    return (lambda: r.draw_geometry(scene, opaque, transparent)), None


def _check_culled(r, scene, opaque, transparent, what, paths=("host", "device", "list", "depth"), modes=("last", "prepass"),
                  instrs=(1, 0), ids=True):
    """every path x mode x instrumentation: the culling pass == the pass without culling; the chunks culled in all"""
    r.sync()  # a deferred clear of the context's own target runs now, not inside the first pass below
    pyr = r.create_depth_pyramid()
    culled = 0
    occluders = opaque[::2]
    n_obj = len(opaque) + (0 if transparent is None else len(transparent))
    for path in paths:
        if path == "list" and n_obj > 16384:  # (svr_create_draw_list's limit)
            continue
        r.set_option(A.OPT_DEVICE_FLATTEN, 1 if path == "device" else (2 if path == "host" else 0))
        draw, lst = _drawer(r, scene, opaque, transparent, path)
        for instr in instrs:
            r.set_option(A.OPT_COUNT_FRAGMENTS, instr)
            r.set_occlusion_pyramid(0)
            want, wst, _ = _pass(r, draw, ids)
            for mode in modes:
                if mode == "last":
                    src = _dev(want["depth"])
                    r.build_depth_pyramid(pyr, src.data_ptr())
                    r.set_occlusion_pyramid(pyr)
                    got, st, ost = _pass(r, draw, ids)
                else:
                    def pre():
                        r.set_occlusion_pyramid(0)
                        r.draw_depth(scene, occluders)
                        r.build_depth_pyramid(pyr)
                        r.set_occlusion_pyramid(pyr)
                        draw()
                    got, st, ost = _pass(r, pre, ids)
                w = f"{what} path={path} mode={mode} instr={instr}"
                _same(got, want, w, st, wst, SAME if instr else ())
                bits = r.read_occlusion()
                culled += int(bits.sum())
                if instr:
                    assert ost.chunks_culled == int(bits.sum()), w
                    assert ost.chunks_tested >= ost.chunks_culled, w
                    assert st.binned_triangles + ost.triangles_culled >= wst.binned_triangles or ost.triangles_culled == 0, w
                r.set_occlusion_pyramid(0)
        if lst is not None:
            lst.close()
    r.set_option(A.OPT_DEVICE_FLATTEN, 0)
    r.destroy_depth_pyramid(pyr)
    return culled


SCEN = sorted(SC.SCENARIOS)


def _capture(lib, name, mp):
    box = {}

    def draw(self, scene, opaque, transparent=None):
        box.update(r=self, scene=scene, opaque=opaque, transparent=transparent)
        raise StopIteration

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        try:
            SC.SCENARIOS[name](lib)
        except StopIteration:
            pass
    return box


@pytest.mark.parametrize("name", SCEN)
def test_scenarios_equal_the_pass_without_culling(hip, name, monkeypatch):
    box = _capture(hip, name, monkeypatch)
    if "r" not in box:
        pytest.fail(f"{name}: no draw_geometry call")
    r = box["r"]
    _check_culled(r, box["scene"], box["opaque"], box["transparent"], name)
    r.close()


@pytest.mark.parametrize("fmt", [A.COLOR_RGBA16F, A.COLOR_RGBA8])
def test_atrium_formats_scissor_interleave(hip, fmt):
    w, h = 192, 108
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64, color_format=fmt)
    _check_culled(r, scene, opaque, transparent, f"atrium fmt={fmt}")
    r.set_scissor(17, 9, 131, 77)
    _check_culled(r, scene, opaque, transparent, "scissor", paths=("host", "list"))
    r.set_scissor(0, 0, w, h)
    r.set_row_interleave(2, 1)
    _check_culled(r, scene, opaque, transparent, "interleave", paths=("host", "device"))
    r.set_row_interleave(1, 0)
    _check_culled(r, scene, opaque, transparent, "no ids", paths=("host",), ids=False)
    r.close()


@pytest.mark.parametrize("name", list(MF.FRAMES))
def test_full_frames(hip, name):
    with open(MF.OUT) as f:
        d = json.load(f)[name]
    w, h, instanced = MF.FRAMES[name]
    kw = dict(camera=S.config5_camera(), instances=S.config5_instances()) if instanced else {}
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=MF.TEX, **kw)
    culled = _check_culled(r, scene, opaque, transparent, name, paths=("host", "device", "depth") if not instanced else ("host", "device"),
                           instrs=(1,))
    assert culled > 0
    # the culled frame against the oracle's digests
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    pyr = r.create_depth_pyramid()
    r.build_depth_pyramid(pyr)
    r.set_occlusion_pyramid(pyr)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    out = T._finish(r)
    assert r.read_occlusion().any()
    for key in ("color", "depth", "rgba8"):
        assert MF.sha(out[key]) == d[key], f"{name}: {key} digest with culling"
    st = out["stats"]
    assert st.triangle_count == d["counters"]["triangle_count"] and st.culled_draws == d["counters"]["culled_draws"]
    r.close()


# ---------------------------------------------------------------- adversarial scenes (identity camera: position = clip)
def _rig(hip, w=64, h=48):
    rig = SC.Rig(hip, w, h)
    return rig, rig.r, rig.material()


def _quad(r, x0, y0, x1, y1, z0, z1=None):
    z1 = z0 if z1 is None else z1
    pos = [(x0, y0, z0), (x1, y0, z1), (x1, y1, z1), (x0, y1, z0)]
    return r.upload_mesh(SC.QUAD_IDX, SC.make_vertices(pos))


def _grid(r, x0, y0, x1, y1, z, n=12, bad=None):
    """n x n quads (2 n^2 triangles: several wave chunks) at depth z; bad: a vertex index set to a non-finite value"""
    xs, ys = np.linspace(x0, x1, n + 1), np.linspace(y0, y1, n + 1)
    pos = np.array([(x, y, z) for y in ys for x in xs], dtype=np.float32)
    if bad is not None:
        pos[bad] = (np.inf, np.nan, z)
    idx = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            idx += [a, a + 1, a + n + 2, a, a + n + 2, a + n + 1]
    idx = np.array(idx, dtype=np.uint32)
    return r.upload_mesh(idx, SC.make_vertices(pos)), idx.size


def _adversarial(hip, kind):
    rig, r, mat = _rig(hip)
    occ = _quad(r, -1, -1, 1, 1, 0.5)
    objs = [SC.render_object(occ, mat, 0, 6)]
    x1 = -0.1 if kind == "beside_the_edge" else 0.9
    hidden, n = _grid(r, -0.9, -0.9, x1, 0.9, 0.2)  # 288 triangles behind the occluder everywhere: culled
    objs.append(SC.render_object(hidden, mat, 0, n))
    if kind == "coplanar_decal":
        m = _quad(r, -0.5, -0.5, 0.5, 0.5, 0.5)  # drawn after the occluder (higher mesh handle): wins the ties
        objs.append(SC.render_object(m, mat, 0, 6))
    elif kind == "touching_box":
        m, k = _grid(r, -0.8, -0.8, 0.8, 0.8, 0.5, n=11)
        objs.append(SC.render_object(m, mat, 0, k))
        m2 = _quad(r, -0.6, -0.6, 0.6, 0.6, 0.3, 0.5)  # a slope that reaches the occluder's depth
        objs.append(SC.render_object(m2, mat, 0, 6))
    elif kind == "beside_the_edge":
        objs[0] = SC.render_object(_quad(r, -1, -1, 0.0, 1, 0.5), mat, 0, 6)  # the occluder covers the left half
        px = 2.0 / 64
        m, k = _grid(r, px, -0.9, 0.9, 0.9, 0.2, n=4)  # one pixel right of its edge, behind its depth
        objs.append(SC.render_object(m, mat, 0, k))
    elif kind == "near_plane":
        wall = _quad(r, -0.5, -0.5, 0.5, 0.5, 0.3, 1.6)  # crosses the near plane (z > w)
        objs.append(SC.render_object(wall, mat, 0, 6))
    elif kind == "non_finite":
        m, k = _grid(r, -0.9, -0.9, 0.9, 0.9, 0.1, n=10, bad=7)  # 200 triangles; vertex 7 is in the first chunk
        objs.append(SC.render_object(m, mat, 0, k))
    opaque = SC.objs(objs)
    return rig, r, SC.identity_scene(), opaque


@pytest.mark.parametrize("kind", ["coplanar_decal", "touching_box", "beside_the_edge", "near_plane", "non_finite"])
def test_adversarial(hip, kind):
    rig, r, scene, opaque = _adversarial(hip, kind)
    empty = SC.objs([])
    culled = _check_culled(r, scene, opaque, empty, kind, modes=("last",))
    assert culled > 0, f"{kind}: the hidden grid is culled"
    # the chunks of the adversarial object itself are never culled
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    pyr = r.create_depth_pyramid()
    want, _, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    src = _dev(want["depth"])
    r.build_depth_pyramid(pyr, src.data_ptr())
    r.set_occlusion_pyramid(pyr)
    _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    bits = r.read_occlusion()
    draws, chunks = r.read_records()
    tri_count = draws[:, 160:164].copy().view(np.uint32)[:, 0]
    hidden_tris = int(opaque[1]["index_count"]) // 3
    for i in np.flatnonzero(bits):
        if kind == "non_finite" and tri_count[chunks[i, 0]] == 200:
            assert chunks[i, 1] != 0, "the chunk with a non-finite vertex was culled"
        else:
            assert tri_count[chunks[i, 0]] == hidden_tris, f"{kind}: chunk {i} of another object was culled"
    r.close()


# ---------------------------------------------------------------- both ends
def test_pyramid_of_zeros_culls_nothing(hip):
    r, scene, opaque, transparent = T.setup_sponza(hip, 160, 90, lod=8, tex_size=64)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    want, wst, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    pyr = r.create_depth_pyramid()
    zeros = _dev(np.zeros((90, 160), np.float32))
    r.build_depth_pyramid(pyr, zeros.data_ptr())
    r.set_occlusion_pyramid(pyr)
    got, st, ost = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    _same(got, want, "zeros", st, wst, ALL)
    assert not r.read_occlusion().any()
    assert ost.chunks_culled == 0 and ost.triangles_culled == 0 and ost.chunks_tested > 0
    r.close()


def _soup(hip, w=160, h=96, n=900, seed=3):
    """a camera with a real perspective and one mesh of n small quads at random depths behind a few big occluders"""
    r = hip.create(w, h)
    mat = r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), r.create_image(S.white_1x1()), r.create_sampler(**S.SAMPLER_LINEAR))
    rng = np.random.default_rng(seed)
    # clusters of 32 quads (a wave chunk is 64 triangles): a chunk's box is small, as in a real mesh
    centres = rng.uniform((-6, -4, -30), (6, 4, -4), (n // 32 + 1, 3))
    c = (np.repeat(centres, 32, axis=0)[:n] + rng.uniform(-0.5, 0.5, (n, 3))).astype(np.float32)
    s = rng.uniform(0.05, 0.4, (n, 1)).astype(np.float32)
    pos = np.concatenate([c + s * np.array(o, np.float32) for o in ((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))], axis=1).reshape(-1, 3)
    idx = (np.arange(n, dtype=np.uint32)[:, None] * 4 + SC.QUAD_IDX[None, :]).reshape(-1)
    soup = r.upload_mesh(idx, SC.make_vertices(pos))
    occ_pos = [(-3, -2, -8), (2, -2, -8), (2, 2.5, -8), (-3, 2.5, -8)]
    occ = r.upload_mesh(SC.QUAD_IDX, SC.make_vertices(occ_pos))
    proj = GL.perspective_rh_zo(GL.radians(70.0), np.float32(w) / np.float32(h), 10000.0, 0.1)
    eye = GL.identity()
    scene = A.scene_struct(eye, proj, proj, [0.1] * 4, (0, 1, 0.5, 1), (1, 1, 1, 1))
    opaque = SC.objs([SC.render_object(occ, mat, 0, 6, extents=(100, 100, 100)),
                      SC.render_object(soup, mat, 0, idx.size, extents=(100, 100, 100))])
    return r, scene, opaque, pos, idx


def _chunk_tris(draws, chunks, i, idx):
    d = draws[chunks[i, 0]]
    tri_count = int(d[160:164].view(np.uint32)[0])
    first_index = int(d[180:184].view(np.uint32)[0])
    mvp = d[64:128].view(np.float32).astype(np.float64).reshape(4, 4)  # column-major: mvp[c] is column c
    t0 = int(chunks[i, 1])
    t1 = min(tri_count, (t0 // 64 + 1) * 64 if first_index % 3 == 0 else t0 + 64)
    tris = idx[first_index:].reshape(-1, 3)[t0:t1]
    return tris, mvp


def test_pyramid_of_ones_and_each_culled_chunk_in_float64(hip):
    w, h = 160, 96
    r, scene, opaque, pos, idx = _soup(hip, w, h)
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    empty = SC.objs([])
    want, wst, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    pyr = r.create_depth_pyramid()
    # (a) soundness, "last": every culled chunk's vertices lie strictly behind the depth over their pixel footprint
    src = _dev(want["depth"])
    r.build_depth_pyramid(pyr, src.data_ptr())
    r.set_occlusion_pyramid(pyr)
    got, st, ost = _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    _same(got, want, "soup last", st, wst)
    bits = r.read_occlusion()
    draws, chunks = r.read_records()
    assert bits.sum() > 0 and ost.chunks_culled == bits.sum()
    depth = want["depth"]
    for i in np.flatnonzero(bits):
        tris, mvp = _chunk_tris(draws, chunks, i, idx)
        p = np.concatenate([pos.astype(np.float64), np.ones((len(pos), 1))], axis=1)
        for tri in tris:
            clip = p[tri] @ mvp  # rows: clip of each corner
            assert (clip[:, 3] > 0).all()
            zw = clip[:, 2] / clip[:, 3]
            xs = (clip[:, 0] / clip[:, 3] + 1) * 0.5 * w
            ys = (clip[:, 1] / clip[:, 3] + 1) * 0.5 * h
            x0, x1 = max(int(np.floor(xs.min())), 0), min(int(np.ceil(xs.max())), w - 1)
            y0, y1 = max(int(np.floor(ys.min())), 0), min(int(np.ceil(ys.max())), h - 1)
            if x0 > x1 or y0 > y1:
                continue
            floor = float(depth[y0:y1 + 1, x0:x1 + 1].min())
            assert zw.max() < floor, f"chunk {i}: a vertex at depth {zw.max()} is not behind {floor}"
    # (b) a pyramid of 1.0 culls every tested chunk whose depth bound is below 1.0: here all of them
    ones = _dev(np.ones((h, w), np.float32))
    r.build_depth_pyramid(pyr, ones.data_ptr())
    _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    ost = r.occlusion_stats()
    bits = r.read_occlusion()
    assert ost.chunks_tested > 0 and bits.sum() == ost.chunks_culled == ost.chunks_tested
    assert 0 < ost.triangles_culled <= len(idx) // 3 + 2
    r.close()


# ---------------------------------------------------------------- effectiveness
def test_culled_share_at_8k_x16(hip):
    w, h = 7680, 4320
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=1, tex_size=64, camera=S.config5_camera(),
                                                   instances=S.config5_instances())
    r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    r.clear_color((1, 1, 1, 1))
    st0 = r.draw_geometry(scene, opaque, transparent)
    pyr = r.create_depth_pyramid()
    r.build_depth_pyramid(pyr)
    r.set_occlusion_pyramid(pyr)
    r.clear_color((1, 1, 1, 1))
    r.draw_geometry(scene, opaque, transparent)
    ost = r.occlusion_stats()
    st = r.get_stats()
    share = ost.triangles_culled / st.triangle_count
    print(f"8k x16 last: chunks tested {ost.chunks_tested} culled {ost.chunks_culled} triangles culled "
          f"{ost.triangles_culled} of {st.triangle_count} ({share:.3f}); binned {st0.binned_triangles} -> {st.binned_triangles}")
    assert share >= CULLED_SHARE_FLOOR
    r.close()


# ---------------------------------------------------------------- ordering
def test_unfenced_prepass_build_culled_pass_with_replay(hip):
    w, h = 192, 108
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    want, _, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    r2, _, _, _ = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    r2.set_option(A.OPT_QUEUE_CAPS, 64)  # every pass overflows at first: the prepass is replayed, then the build
    pyr = r2.create_depth_pyramid()

    def seq():
        r2.draw_depth(scene, opaque[::2])
        r2.build_depth_pyramid(pyr)
        r2.set_occlusion_pyramid(pyr)
        r2.draw_geometry(scene, opaque, transparent)
    got, st, _ = _pass(r2, seq)
    assert st.replayed_passes > 0
    _same(got, want, "replayed prepass")
    r2.close()
    r.close()


def test_replayed_prepass_and_build_really_cull(hip):
    """the same sequence on a scene where the prepass hides most chunks: the build was replayed from the replayed prepass
    (the pyramid equals numpy's of that depth) and the culling pass, replayed behind it, culled against it"""
    w, h = 160, 96
    r, scene, opaque, _, _ = _soup(hip, w, h)
    empty = SC.objs([])
    want, wst, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, empty))
    pre, _, _ = _pass(r, lambda: r.draw_depth(scene, opaque[:1]))  # the occluder's depth alone
    r2, _, _, _, _ = _soup(hip, w, h)
    r2.set_option(A.OPT_QUEUE_CAPS, 64)  # the prepass and the culling pass overflow at first and are replayed
    r2.set_option(A.OPT_COUNT_FRAGMENTS, 1)
    pyr = r2.create_depth_pyramid()

    def seq():
        r2.draw_depth(scene, opaque[:1])
        r2.build_depth_pyramid(pyr)
        r2.set_occlusion_pyramid(pyr)
        r2.draw_geometry(scene, opaque, empty)
    got, st, ost = _pass(r2, seq)
    assert st.replayed_passes > 0
    _same(got, want, "replayed prepass, soup")
    bits = r2.read_occlusion()
    assert bits.any() and ost.chunks_culled == int(bits.sum()), "the replayed culling pass culled nothing"
    _check_pyramid(r2, pyr, pre["depth"], "pyramid of the replayed prepass")
    r2.close()
    r.close()


def test_rebuild_between_two_passes(hip):
    w, h = 160, 90
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    pyr = r.create_depth_pyramid()
    ones = _dev(np.ones((h, w), np.float32))
    zeros = _dev(np.zeros((h, w), np.float32))
    plain, _, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    r.build_depth_pyramid(pyr, ones.data_ptr())
    r.set_occlusion_pyramid(pyr)
    all_culled, _, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    assert not np.array_equal(all_culled["depth"], plain["depth"])
    # unfenced: build(zeros), pass 1, build(ones), pass 2 into other targets, build(zeros) again
    ta, tb = _targets(r, False, 5), _targets(r, False, 5)
    r.build_depth_pyramid(pyr, zeros.data_ptr())
    r.bind_targets(ta[0].data_ptr(), ta[1].data_ptr())
    r.draw_geometry(scene, opaque, transparent)
    r.build_depth_pyramid(pyr, ones.data_ptr())
    r.bind_targets(tb[0].data_ptr(), tb[1].data_ptr())
    r.draw_geometry(scene, opaque, transparent)
    r.build_depth_pyramid(pyr, zeros.data_ptr())
    r.sync()
    torch.cuda.synchronize()
    T.assert_images_identical(ta[1].cpu().numpy(), plain["depth"], "pass 1 sees the pyramid of zeros")
    T.assert_images_identical(ta[0].cpu().numpy(), plain["color"], "pass 1 colour")
    T.assert_images_identical(tb[1].cpu().numpy(), all_culled["depth"], "pass 2 sees the pyramid of ones")
    T.assert_images_identical(tb[0].cpu().numpy(), all_culled["color"], "pass 2 colour")
    r.bind_targets(None, None)
    # destroying a bound pyramid unbinds it: the next pass draws everything
    r.destroy_depth_pyramid(pyr)
    again, _, _ = _pass(r, lambda: r.draw_geometry(scene, opaque, transparent))
    _same(again, {k: plain[k] for k in ("color", "depth")}, "after destroy")
    r.close()


# ---------------------------------------------------------------- refusals
def test_multiview_and_handles_are_refused(hip):
    w, h = 64, 48
    r, scene, opaque, transparent = T.setup_sponza(hip, w, h, lod=8, tex_size=64)
    pyr = r.create_depth_pyramid()
    assert pyr == 1
    r.set_occlusion_pyramid(pyr)
    color = torch.zeros((2, h, w, 4), dtype=torch.int16, device="cuda")
    depth = torch.zeros((2, h, w), dtype=torch.float32, device="cuda")
    with pytest.raises(pkg.SvrError, match="multiview") as e:
        r.draw_views([scene, scene], color.data_ptr(), depth.data_ptr(), opaque, transparent)
    assert e.value.code == -5
    with pytest.raises(pkg.SvrError) as e:
        r.draw_depth_views([scene, scene], depth.data_ptr(), opaque)
    assert e.value.code == -5
    r.set_occlusion_pyramid(0)
    r.draw_views([scene, scene], color.data_ptr(), depth.data_ptr(), opaque, transparent)
    for bad in (0, 2, 99):
        with pytest.raises(pkg.SvrError) as e:
            r.build_depth_pyramid(bad)
        assert e.value.code == -4
        with pytest.raises(pkg.SvrError) as e:
            r.read_depth_pyramid(bad, 1)
        assert e.value.code == -4
    with pytest.raises(pkg.SvrError) as e:
        r.set_occlusion_pyramid(7)
    assert e.value.code == -4
    n = r.pyramid_levels(pyr)
    assert n == 6
    for level in (0, n + 1):
        with pytest.raises(pkg.SvrError, match="level out of range"):
            r.read_depth_pyramid(pyr, level)
    r.destroy_depth_pyramid(pyr)
    with pytest.raises(pkg.SvrError) as e:
        r.destroy_depth_pyramid(pyr)
    assert e.value.code == -4
    r.close()
