"""The hierarchical-depth-test scenarios (scenarios.HIZ_GEOMETRY) test what their names say, checked on the CPU oracle
with numpy doing the geometry: every tile they aim at holds enough opaque triangles for the test (more than 64 for
scan_columns, 128 for a split tile's quarters, 1024 for tile_body's filter), and the pixels each scene is built around
show the layer they must.  A scene that stops reaching its target fails here, not silently on the GPU."""
import numpy as np
import pytest

import scenarios as SC
import svr_testlib as T

f32 = np.float32


def bin_depths(sc):
    """{(tx, ty): opaque triangles whose pixel box overlaps the tile}, with the oracle's box rule (24.8 snap, box of the
    pixel centres inside, clamped to the frame and the scissor).  Triangles the clipper cuts count once, by their box."""
    sx, sy, sw, sh = sc.scissor if sc.scissor else (0, 0, sc.w, sc.h)
    counts = {}
    for layer in sc.layers:
        t = layer.tris
        X, Y = np.rint(t[:, :, 0] * 256).astype(np.int64), np.rint(t[:, :, 1] * 256).astype(np.int64)
        x0 = np.maximum((X.min(1) + 127) >> 8, sx)
        x1 = np.minimum((X.max(1) - 128) >> 8, sx + sw - 1)
        y0 = np.maximum((Y.min(1) + 127) >> 8, sy)
        y1 = np.minimum((Y.max(1) - 128) >> 8, sy + sh - 1)
        ok = (x0 <= x1) & (y0 <= y1)
        for a, b, c, d in zip(x0[ok], x1[ok], y0[ok], y1[ok]):
            for ty in range(c // 32, d // 32 + 1):
                for tx in range(a // 32, b // 32 + 1):
                    counts[(tx, ty)] = counts.get((tx, ty), 0) + 1
    return counts


@pytest.fixture(scope="module")
def frames(oracle):
    return {name: SC.SCENARIOS[name](oracle) for name in SC.HIZ_GEOMETRY}


def tile(a, tx, ty):
    return a[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32]


def dominant(color):
    """index of the largest of r, g, b per pixel (the scenes' layers are pure red, green or blue, lit)"""
    return np.argmax(T.f16_bits_to_f32(color)[..., :3], axis=-1)


MIN_BIN = {"hiz_occluder_edges": 128, "hiz_occluder_edges_rgba8": 128, "hiz_depth_margins": 128,
           "hiz_deep_opaque_65": 64, "hiz_deep_opaque_129": 128, "hiz_deep_opaque_1025": 1024,
           "hiz_deep_opaque_2100": 2048, "hiz_clipped_occluders": 1024, "hiz_depth_extremes": 64,
           "hiz_deep_opaque_odd_size": 1024, "hiz_deep_opaque_scissor": 1024, "hiz_deep_opaque_rgba8": 256}


def test_every_scene_is_listed():
    assert set(MIN_BIN) == set(SC.HIZ_GEOMETRY)
    assert set(SC.HIZ_GEOMETRY) <= set(SC.SCENARIOS)


@pytest.mark.parametrize("name", sorted(SC.HIZ_GEOMETRY))
def test_aimed_tiles_are_deep_enough(name):
    sc = SC.HIZ_GEOMETRY[name]()
    counts = bin_depths(sc)
    if name.startswith("hiz_occluder_edges"):
        aimed = [(ox // 32, oy // 32) for ox, oy in map(SC.edge_slot_origin, range(len(SC.EDGE_SLOTS)))]
    elif name in ("hiz_depth_margins", "hiz_depth_extremes", "hiz_clipped_occluders"):
        aimed = SC.SLOTS
    else:
        aimed = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for t in aimed:
        assert counts.get(t, 0) > MIN_BIN[name], f"{name} tile {t}: {counts.get(t, 0)} triangles"
    # the draw list's fast path (4096 objects) and the object caps the ID and draw-list tests assume
    assert len(sc.layers) <= 4096


def test_occluder_edges_show_the_back_quad_on_excluded_edges(frames):
    for name in ("hiz_occluder_edges", "hiz_occluder_edges_rgba8"):
        depth = frames[name]["depth"]
        excluded_seen = 0
        for k, ((cx, cy), off, flip) in enumerate(SC.EDGE_SLOTS):
            ox, oy = SC.edge_slot_origin(k)
            d = depth[oy:oy + 32, ox:ox + 32]
            r0, c0 = (31 if cy else 0), (31 if cx else 0)
            inner = np.delete(np.delete(d, r0, axis=0), c0, axis=1)
            assert np.all(inner == f32(SC.EDGE_Z_FRONT)), (name, k)
            # top-left rule: a leg along the first row is a top edge, along the first column a left edge (included)
            row_in = off > 0 or (off == 0 and cy == 0)
            col_in = off > 0 or (off == 0 and cx == 0)
            rest = [c for c in range(32) if c != c0]
            want_row = f32(SC.EDGE_Z_FRONT if row_in else SC.EDGE_Z_BACK)
            want_col = f32(SC.EDGE_Z_FRONT if col_in else SC.EDGE_Z_BACK)
            assert np.all(d[r0, rest] == want_row), (name, k, d[r0, rest])
            assert np.all(np.delete(d[:, c0], r0) == want_col), (name, k)
            excluded_seen += (not row_in) + (not col_in)
        assert excluded_seen >= 8


def test_depth_margins_ties_go_to_the_later_layer(frames):
    sc = SC.hiz_depth_margins_geometry()
    depth, dom = frames["hiz_depth_margins"]["depth"], dominant(frames["hiz_depth_margins"]["color"])
    for k, kind in enumerate(SC.MARGIN_KINDS):
        tx, ty = SC.SLOTS[k]
        d, c = tile(depth, tx, ty), tile(dom, tx, ty)
        zmin = SC._plane_min_depth(SC._front_plane(kind, 32 * tx, 32 * ty), 32 * tx, 32 * ty)
        at_min = d == zmin
        assert at_min.any(), kind
        assert np.all(c[at_min] == 2), kind  # the layer at the front's smallest depth, drawn last, wins where it ties
        if kind == "constant":
            assert at_min.all()
        elif kind == "slivers":  # the slivers one ulp in front show, the ones at and behind the front do not
            above = d == np.nextafter(zmin, f32(1))
            assert above.sum() >= 8 and np.all(at_min | above)
        else:  # the sloped planes: the later copy of the front (GREEN) wins everywhere else, nothing behind shows
            assert (~at_min).sum() > 900 and np.all(c[~at_min] == 1) and np.all(d >= zmin), kind
    assert sc.layers[-1].color == SC.BLUE


def test_deep_stacks_show_their_nearest_layer(frames):
    for name in ("hiz_deep_opaque_65", "hiz_deep_opaque_129", "hiz_deep_opaque_1025", "hiz_deep_opaque_2100",
                 "hiz_deep_opaque_rgba8"):
        depth = frames[name]["depth"]
        for tx, ty in ((0, 0), (1, 0), (0, 1)):
            assert np.all(tile(depth, tx, ty) == f32(SC.DEEP_FRONT_Z)), (name, tx, ty)
        d3 = tile(depth, 1, 1)
        assert np.all(d3[:, :16] == f32(SC.DEEP_FRONT_Z)) and np.all(d3[:, 16:] < f32(SC.DEEP_FRONT_Z)), name
    # tile 2's two fronts: the later copy wins (its colour, not the first copy's)
    sc = SC.hiz_deep_opaque_geometry(1050)
    first, last = sc.layers[2].color, sc.layers[1048].color
    got = T.f16_bits_to_f32(tile(frames["hiz_deep_opaque_2100"]["color"], 0, 1))[..., :3]
    g = got.reshape(-1, 3).mean(0)
    assert np.dot(g / np.linalg.norm(g), np.array(last[:3]) / np.linalg.norm(last[:3])) > \
        np.dot(g / np.linalg.norm(g), np.array(first[:3]) / np.linalg.norm(first[:3]))
    # in tile 0 of the 2100 stack the front lies in the second filter window (entries 1024 ..), in tile 1 in the first
    for (tx, ty), window in (((0, 0), 1), ((1, 0), 0)):
        entries = [t for layer in sc.layers for t in layer.tris
                   if t[:, 0].min() < 32 * tx + 32 and t[:, 0].max() > 32 * tx and t[:, 1].min() < 32 * ty + 32 and t[:, 1].max() > 32 * ty]
        first_front = next(i for i, t in enumerate(entries) if t[0, 2] == SC.DEEP_FRONT_Z)
        assert first_front // 1024 == window, (tx, ty, first_front)


def test_scissor_and_odd_size_stacks(frames):
    d = frames["hiz_deep_opaque_scissor"]["depth"]
    x, y, w, h = 5, 11, 50, 40
    outside = np.ones_like(d, dtype=bool)
    outside[y:y + h, x:x + w] = False
    assert np.all(d[outside] == 0) and np.all(d[~outside] > 0)
    assert np.all(d[y:32, x:32] == f32(SC.DEEP_FRONT_Z))
    d = frames["hiz_deep_opaque_odd_size"]["depth"]
    assert d.shape == (45, 53) and np.all(d[:32, :32] == f32(SC.DEEP_FRONT_Z))


def test_clipped_occluders_are_cut(frames):
    depth = frames["hiz_clipped_occluders"]["depth"]
    front = depth >= f32(0.8)
    for tx, ty in SC.SLOTS[:3]:
        assert tile(front, tx, ty).all(), (tx, ty)
    cut = tile(front, *SC.SLOTS[3])
    assert cut[:, :20].all() and not cut[:, 24:].any()  # the near plane cuts slot 3 at x = 21.8: the stack shows beyond
    assert depth.max() <= 1.0


def test_depth_extremes(frames):
    f = frames["hiz_depth_extremes"]
    depth, dom = f["depth"], dominant(f["color"])
    assert not np.any(depth.view(np.uint32) == 0x80000000)  # never -0.0 (C5)
    assert np.all(tile(depth, 0, 0) == 1.0) and np.all(tile(dom, 0, 0) == 1)
    for (tx, ty), want in zip(SC.SLOTS[1:], (1, 1, 0)):  # ties at 0.0: the later layer wins
        zero = tile(depth, tx, ty) == 0
        assert zero.sum() > 512 and np.all(tile(dom, tx, ty)[zero] == want), (tx, ty)
