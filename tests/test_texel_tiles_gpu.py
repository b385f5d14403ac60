"""The texel arena stores every mip level in tiles (csrc/svr_device.h texel_offset).  Nothing a caller sees may tell:
levels read back as linear rows, and frames sample the same texels.  Extents below, at and across a tile, strongly
non-square ones (the layout's tail past the smaller extent), power-of-two and not; uv running -1.5 .. 2.5 so that
footprints cross the wrap seam and every tile seam; every filter and mip mode, hence the fragment stage's COMMON path
(LINEAR/LINEAR/MIPMAP_LINEAR on power-of-two extents) and its generic one.  Everything bit for bit against the oracle."""
import numpy as np
import pytest

import __graft_entry__ as g
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A, S = pkg.abi, pkg.scenes
pytestmark = pytest.mark.gpu

EXTENTS = [(1, 1), (2, 2), (5, 3), (8, 4), (9, 5), (33, 17), (64, 64), (1024, 4), (4, 1024)]  # (w, h)
SAMPLERS = {
    "linear_mip_linear": dict(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=0.0, max_lod=1000.0),
    "linear_mip_nearest": dict(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_NEAREST, min_lod=0.0, max_lod=1000.0),
    "nearest_mip_linear": dict(mag=A.FILTER_NEAREST, minf=A.FILTER_NEAREST, mip=A.MIPMAP_LINEAR, min_lod=0.0, max_lod=1000.0),
    "nearest_mip_nearest": dict(mag=A.FILTER_NEAREST, minf=A.FILTER_NEAREST, mip=A.MIPMAP_NEAREST, min_lod=0.0, max_lod=1000.0),
    # held to the two largest levels: minified footprints stride over all of their tiles
    "linear_mip_linear_lod_0_1": dict(mag=A.FILTER_LINEAR, minf=A.FILTER_LINEAR, mip=A.MIPMAP_LINEAR, min_lod=0.0, max_lod=0.75),
}
_TEXTURES = {}


def texture(w, h):
    if (w, h) not in _TEXTURES:
        _TEXTURES[(w, h)] = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    return _TEXTURES[(w, h)]


def levels_of(w, h):
    return int(np.floor(np.log2(max(w, h)))) + 1


def uv_quad():
    """the whole target, uv from -1.5 to 2.5 either way"""
    pos = [(-1, -1, 0.5), (1, -1, 0.5), (1, 1, 0.5), (-1, 1, 0.5)]
    uv = [(-1.5, -1.5), (2.5, -1.5), (2.5, 2.5), (-1.5, 2.5)]
    return SC.make_vertices(pos, [(0, 1, 0)] * 4, uv, [(1, 1, 1, 1)] * 4)


def frames(r, images, sampler):
    """one 64 x 64 frame per image: its quad through mesh.frag with this sampler"""
    mesh = r.upload_mesh(SC.QUAD_IDX, uv_quad())
    smp = r.create_sampler(**sampler)
    out = []
    for img in images:
        mat = r.write_material(A.PASS_MAIN_COLOR, (1, 1, 1, 1), img, smp)
        r.clear_color((0, 0, 0, 1))
        r.draw_geometry(SC.identity_scene(), SC.objs([SC.render_object(mesh, mat, 0, 6)]))
        r.sync()
        out.append(r.read_color().copy())
    return out


@pytest.mark.parametrize("w,h", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
def test_levels_round_trip(hip, oracle, w, h):
    chains = []
    for lib in (hip, oracle):
        r = lib.create(8, 8)
        img = r.create_image(texture(w, h), mipmapped=True)
        chains.append([r.read_image_level(img, l) for l in range(levels_of(w, h))])
        with pytest.raises(A.SvrError):
            r.read_image_level(img, levels_of(w, h))
        r.close()
    assert np.array_equal(chains[0][0], texture(w, h))
    for l, (x, y) in enumerate(zip(*chains)):
        assert x.shape == (max(1, h >> l), max(1, w >> l), 4), f"{w}x{h} level {l}: {x.shape}"
        assert np.array_equal(x, y), f"{w}x{h} level {l}"


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_quads_across_the_seams(hip, oracle, name):
    got = []
    for lib in (hip, oracle):
        r = lib.create(64, 64)
        images = [r.create_image(texture(w, h), mipmapped=True) for (w, h) in EXTENTS]
        got.append(frames(r, images, SAMPLERS[name]))
        r.close()
    for (w, h), a, b in zip(EXTENTS, *got):
        T.assert_images_identical(a, b, f"{name}, {w}x{h}")
    assert len({a.tobytes() for a in got[0]}) == len(EXTENTS), "every image gives a frame of its own"


def test_after_the_arena_grew_and_a_hole_was_reused(hip, oracle):
    """The images of the list, placed before the arena grows, across the growth and into the hole a destroyed image leaves."""
    big = np.random.default_rng(7).integers(0, 256, (2048, 2048, 4), dtype=np.uint8)   # 22 MiB with its levels
    r = hip.create(64, 64)
    before = [r.create_image(texture(w, h), mipmapped=True) for (w, h) in EXTENTS[:5]]
    pad = [r.create_image(big, mipmapped=True) for _ in range(3)]                      # past the arena's first 64 MiB
    after = [r.create_image(texture(w, h), mipmapped=True) for (w, h) in EXTENTS[5:7]]
    r.destroy_image(pad[1])
    hole = [r.create_image(texture(w, h), mipmapped=True) for (w, h) in EXTENTS[7:]]   # first fit: inside the hole
    images = before + after + hole
    for (w, h), img in zip(EXTENTS, images):
        assert np.array_equal(r.read_image_level(img, 0), texture(w, h)), f"{w}x{h}"
    assert np.array_equal(r.read_image_level(pad[2], 0), big)
    got = frames(r, images, SAMPLERS["linear_mip_linear"])
    r.close()
    ro = oracle.create(64, 64)
    want = frames(ro, [ro.create_image(texture(w, h), mipmapped=True) for (w, h) in EXTENTS], SAMPLERS["linear_mip_linear"])
    ro.close()
    for (w, h), a, b in zip(EXTENTS, got, want):
        T.assert_images_identical(a, b, f"{w}x{h}")
