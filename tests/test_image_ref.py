"""The CPU oracle's stores, transparent blend, mip generation and blit against tests/image_ref.py, the independent exact
statement of those rules; tests/test_image_ref_gpu.py holds the HIP library to the same checkers.

The oracle owns its targets (svr_bind_targets is refused), so a destination is built here with one-row scissored clears
(a clear covers whole rows of the scissor) and opaque quads of the exact kind drawn in the same pass; what the target
then holds is stated by S1 from the values handed in, not read back.

The share of pixels offered either way depends on the reference and the inputs alone and is asserted here, on the CPU:
at most EITHER_OR_CAP of a case's checked pixels.  With exact sources it is 0 for every RGBA16F blend case.

Every deliberately wrong variant of the reference (image_ref.VARIANTS) must disagree with the oracle on these cases.

`python tests/test_image_ref.py` (repository root on PYTHONPATH) prints the figures of DESIGN.md §2's table."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import image_cases as IC
import image_ref as IR

A = IC.A
f32 = np.float32
FMT_IDS = list(IC.FORMATS)


# ---------------------------------------------------------------- 1. stores
def test_half_conversions(oracle):
    L = oracle.lib
    for bits in range(65536):
        want, got = IR.half_value(bits), L.svr_oracle_f16_to_f32(bits)
        assert (got != got) if want != want else (Fr(got) == want if not isinstance(want, float) else got == want), hex(bits)
    assert np.signbit(f32(L.svr_oracle_f16_to_f32(0x8000))) and not np.signbit(f32(L.svr_oracle_f16_to_f32(0)))
    for v in IC.store_probe_floats().tolist():
        if v == 0.0:  # (a rational has no signed zero: both zeros are asserted below)
            continue
        assert L.svr_oracle_f32_to_f16(v) == IR.store_f16_one(Fr(v)), v
    assert L.svr_oracle_f32_to_f16(float("inf")) == 0x7c00 and L.svr_oracle_f32_to_f16(float("-inf")) == 0xfc00
    assert L.svr_oracle_f32_to_f16(-0.0) == 0x8000 and L.svr_oracle_f32_to_f16(0.0) == 0 and L.svr_oracle_f32_to_f16(-2.0 ** -26) == 0x8000


def test_array_stores_agree_with_the_rational_ones():
    probes = IC.store_probe_floats()[::7]
    got = IR.store_np(probes, IR.RGBA16F)
    for v, g in zip(probes.tolist(), got.tolist()):
        if v != 0.0:
            want = IR.half_value(IR.store_f16_one(Fr(v)))
            assert g == want, v
    vals = np.concatenate([np.array([c for c, _ in IC.unorm8_tie_floats()]), np.random.default_rng(3).uniform(-0.5, 1.5, 2000)])
    got = IR.store_np(vals, IR.RGBA8)
    for v, g in zip(vals.tolist(), got.tolist()):
        assert g == IR.store_un8_one(Fr(v)), v


def clear_rows(r, rows):
    """rows[y] = the four floats row y is cleared to"""
    for y, rgba in enumerate(rows):
        r.set_scissor(0, y, r.width, 1)
        r.clear_color(tuple(float(v) for v in rgba))
    r.set_scissor(0, 0, r.width, r.height)


def test_stores_through_row_clears(oracle):
    """256 rows x 4 channels of binary32 values through the fp16 store, read back raw, as bytes and through the identity
    blit in both channel orders; among them both infinities and a NaN row, which the rows beside them must not feel"""
    probes = IC.store_probe_floats()
    rng = np.random.default_rng(5)
    vals = rng.choice(probes, (256, 4)).astype(f32)
    vals[:8] = np.array([[1.0, 0.5, 0.25, 1.0], [np.inf, 1.0, -np.inf, 0.5], [0.5, 65520.0, 2.0, 1.0], [np.nan, 0.25, 0.75, np.nan],
                         [0.75, np.inf, 0.1, 0.2], [IC.MID_LOW, IC.MID_HIGH, 127.5 / 255, 0.5], [-0.0, 0.0, -1e-9, 1e-9], [0.3, 0.6, 0.9, 1.0]], f32)
    r = oracle.create(256, 256, A.COLOR_RGBA16F)
    clear_rows(r, vals)
    want16 = np.zeros((256, 4), np.uint16)
    for y in range(256):
        for c in range(4):
            v = float(vals[y, c])
            want16[y, c] = 0x7e00 if v != v else (0x8000 if np.signbit(v) else 0) if v == 0 else IR.store_f16_one(v if np.isinf(v) else Fr(v))
    got = r.read_color()
    nan = np.isnan(vals)
    assert np.all(np.isnan(got.view(np.float16)[:, 0, :][nan])) and np.array_equal(got[:, 0, :][~nan], want16[~nan])
    assert np.all(got == got[:, :1, :])
    table = IC.half_to_un8_table()
    want8 = np.repeat(table[got[:, 0, :]][:, None, :], 256, axis=1)
    assert np.array_equal(r.read_color(as_rgba8=True), want8)
    for fmt in (A.SWAPCHAIN_B8G8R8A8, A.SWAPCHAIN_R8G8B8A8):
        assert np.array_equal(r.read_swapchain(256, 256, fmt), IC.swizzle(want8, fmt)), f"identity blit, format {fmt}"
    r.close()


def test_unorm8_store_through_row_clears(oracle):
    """an RGBA8 target: binary32 values through the UNORM8 store, among them products c * 255 that land on k + 1/2"""
    ties = IC.unorm8_tie_floats()
    rng = np.random.default_rng(6)
    vals = rng.uniform(-0.25, 1.25, (64, 4)).astype(f32)
    for i, (c, _) in enumerate(ties):
        vals[i % 64, i % 4] = c
    vals[40] = (np.nan, np.inf, -np.inf, -0.0)
    r = oracle.create(16, 64, A.COLOR_RGBA8)
    clear_rows(r, vals)
    got = r.read_color()
    for y in range(64):
        for c in range(4):
            v = float(vals[y, c])
            assert int(got[y, 3, c]) == IR.store_un8_one(v if (v != v or np.isinf(v)) else Fr(v)), (y, c, v)
    r.close()


# ---------------------------------------------------------------- 2. blending
def oracle_rows(fmt, h=IC.BLEND_H, seed=17):
    """the colours the rows of the oracle's destination are cleared to: zeros, half subnormals, [0, 1], negative, large
    values, alphas among 0, 2^-14, 1/2, 1, 2, 65504; rows 30 - 33 the double-rounding rows (dst * dst.a = +-2^-28)"""
    rng = np.random.default_rng(seed + fmt)
    rows = np.zeros((h, 4), f32)
    alphas = [0.0, IC.TINY, 0.5, 1.0, 2.0, 65504.0] if fmt == A.COLOR_RGBA16F else [0.0, 1 / 255, 0.5, 254 / 255, 1.0, 0.7]
    for y in range(h):
        kind = y % 6
        rgb = [np.zeros(3), rng.integers(1, 1024, 3) * 2.0 ** -24, rng.uniform(0, 1, 3), -rng.uniform(0, 4, 3), rng.uniform(0, 65504, 3), rng.uniform(0, 2, 3)][kind]
        if fmt == A.COLOR_RGBA8:
            rgb = np.clip(np.abs(rgb), 0, 1) if kind != 4 else rng.uniform(0, 1, 3)
        rows[y, :3], rows[y, 3] = rgb, alphas[(y // 6 + y) % 6]
    if fmt == A.COLOR_RGBA16F:
        for y in range(30, min(34, h)):
            s = 1.0 if y % 2 == 0 else -1.0
            rows[y] = (s * IC.TINY, -s * IC.TINY, s * IC.TINY, IC.TINY)
    return rows


OPAQUE = (IC.Layer((8, 20, 24, 44), 0.5, (0.25, 0.5, 0.75, 1)), IC.Layer((34, 26, 50, 38), 0.625, (0.1, 0.9, 0.3, 1)),
          IC.Layer((40, 10, 60, 34), 0.25, (1.5, 0.0, 2.0 ** -20, 1)))


def oracle_destination(fmt, rows, opaque, w=IC.BLEND_W, h=IC.BLEND_H):
    """what the target holds after the row clears and the opaque quads, by S1; the quads of a pass start from depth 0 and
    win at depth >= the depth before them"""
    codes = np.zeros((h, w, 4), np.uint16 if fmt == A.COLOR_RGBA16F else np.uint8)
    for y in range(h):
        codes[y, :, :] = [next(iter(IR.store(Fr(float(v)), Fr(0), fmt))) for v in rows[y]]
    depth = np.zeros((h, w), f32)
    for l in opaque:
        m = IC.layer_coverage(l, w, h) & (f32(l.z) >= depth)
        depth[m] = f32(l.z)
        codes[m] = [next(iter(IR.store(Fr(v), Fr(0), fmt))) for v in l.rgba[:3] + (1.0,)]
    return codes, depth


_BLEND = {}


def oracle_blend(oracle, k_layers, fmt, scissor=None):
    """(the oracle's colour codes and depth, the destination by S1, the layers), made once"""
    key = (k_layers, fmt, scissor)
    if key not in _BLEND:
        w, h = IC.BLEND_W, IC.BLEND_H
        rows, layers = oracle_rows(fmt), IC.blend_layers(k_layers, fmt)
        IC.exact_source(list(OPAQUE) + layers)
        r = oracle.create(w, h, fmt)
        clear_rows(r, rows)
        if scissor:
            r.set_scissor(*scissor)
        r.draw_geometry(IC.blend_scene(), IC.layer_objects(r, OPAQUE, w, h, transparent=False), IC.layer_objects(r, layers, w, h))
        got = (r.read_color(), r.read_depth())
        r.close()
        codes, depth = oracle_destination(fmt, rows, OPAQUE)
        if scissor:  # the opaque quads are cut by the scissor too: outside it the rows stay as cleared
            sx, sy, sw, sh = scissor
            inside = np.zeros((h, w), bool)
            inside[sy:sy + sh, sx:sx + sw] = True
            rows_only, _ = oracle_destination(fmt, rows, ())
            codes[~inside], depth[~inside] = rows_only[~inside], 0.0
        _BLEND[key] = (got, codes, depth, IC.reference_layers(layers, w, h))
    return _BLEND[key]


BLEND_CASES = [(k, s) for k in (1, 3, 8, 70) for s in (None, IC.SCISSOR)]


@pytest.mark.parametrize("fmt", FMT_IDS)
@pytest.mark.parametrize("k_layers,scissor", BLEND_CASES, ids=[f"K{k}{'-scissor' if s else ''}" for k, s in BLEND_CASES])
def test_blend(oracle, k_layers, scissor, fmt):
    (color, depth), codes, seed_depth, layers = oracle_blend(oracle, k_layers, IC.FORMATS[fmt], scissor)
    ref = IR.blend_pass(codes, seed_depth, layers, IC.FORMATS[fmt], scissor)
    worst = [0.0]
    n, offered = IC.check_blend(f"oracle K={k_layers} {fmt}", color, depth, codes, seed_depth, ref, worst)
    blended = len(ref.sets)
    print(f"K={k_layers} {fmt} scissor={scissor}: {n} pixels checked, {blended} blended, {offered} offered"
          + (f", worst error / allowance {worst[0]:.3f}" if fmt == "rgba8" else ""))
    assert fmt != "rgba8" or 0.0 < worst[0] <= 1.0
    assert blended >= 32 * 8 and offered <= IC.EITHER_OR_CAP * n
    if fmt == "rgba16f":
        assert offered == 0, "exact sources leave an RGBA16F blend no choice"


def test_blend_cases_reach_what_they_name(oracle):
    """the depth test decides both ways and at equality; sums overflow to infinity; the double-rounding pixels are there"""
    (color, _), codes, depth, layers = oracle_blend(oracle, 8, A.COLOR_RGBA16F)
    zs = {l[1] for l in layers}
    cov = np.any([l[0] for l in layers], axis=0)
    assert any((depth[cov] == f32(z)).any() for z in zs) and any((depth[cov] > f32(z)).any() for z in zs) and any((depth[cov] < f32(z)).any() for z in zs)
    assert (color[cov] == 0x7c00).any(), "a sum overflowed to infinity"
    (color1, _), codes1, _, _ = oracle_blend(oracle, 1, A.COLOR_RGBA16F)
    craft = color1[30:34, 24:34]  # the double-rounding rows, between the opaque quads
    assert set(np.unique(craft[..., 0]).tolist()) == {0x3c00} and set(np.unique(craft[..., 1]).tolist()) == {0x3c02}, \
        "the half-way sums are rounded twice: to the half-way binary32 value, then to the even half"


def blend_cap_hip(fmt):
    """the offered share of the HIP library's blend cases (a seeded destination): depends on the reference and the inputs
    alone, so it is computed here; -> {(K, scissor): (pixels, blended, offered)}"""
    out = {}
    color, depth = IC.seeded_target(fmt)
    for k, s in BLEND_CASES:
        ref = IR.blend_pass(color, depth, IC.reference_layers(IC.blend_layers(k, fmt), IC.BLEND_W, IC.BLEND_H), fmt, s)
        out[(k, s)] = (depth.size, len(ref.sets), sum(any(len(c) > 1 for c in sets) for sets in ref.sets.values()))
    return out


@pytest.mark.parametrize("fmt", FMT_IDS)
def test_blend_either_or_cap_of_the_seeded_destination(fmt):
    for (k, s), (n, blended, offered) in blend_cap_hip(IC.FORMATS[fmt]).items():
        print(f"seeded destination K={k} {fmt} scissor={s}: {n} pixels, {blended} blended, {offered} offered")
        assert offered <= IC.EITHER_OR_CAP * n, f"K={k} {fmt} scissor={s}: {offered} of {n} pixels offered"
        if fmt == "rgba16f":
            assert offered == 0


# ---------------------------------------------------------------- 3. mip generation
@pytest.mark.parametrize("content", IC.MIP_CONTENTS)
def test_mip_chain(oracle, content):
    r = oracle.create(8, 8)
    n = sum(IC.check_mip_chain(r, w, h, content) for w, h in IC.MIP_EXTENTS)
    r.close()
    print(f"{content}: {n} texels over {len(IC.MIP_EXTENTS)} chains")


def test_tie_textures_hold_ties_of_both_parities():
    """the 'ties' content: exact k + 1/2 sums with k even and k odd, on the 2:1 weights and on 5 -> 2 (quarters), 7 -> 3
    (thirds) and 3 -> 1 (the centre texel alone, weights 1 and 0).  Thirds alone never sum to k + 1/2 and the centre
    alone never rounds, so 7 -> 3 ties through its other axis (7 x 5) and 3 -> 1 through 5 x 3; 1 x 7 cannot tie at all"""
    for (w, h) in ((2, 1), (5, 3), (7, 5), (8, 4), (9, 5), (16, 16), (17, 9), (33, 17), (31, 64), (64, 1)):
        even, odd = IC.tie_counts(IC.mip_texture(w, h, "ties"))
        assert even and odd, f"{w}x{h}: ties on even quotients {even}, on odd {odd}"


def test_raster_cases_textures_follow_the_rule(oracle):
    """raster_cases.mip_chain_by_rule: the chains families C and D sample are image_ref's, whoever read them back"""
    import raster_cases as RC
    rig = RC.Rig(oracle, 64, 48)
    for case in RC.cases("C"):
        rig.material(case)
        RC.mip_chain_by_rule(case)
    rig.close()


# ---------------------------------------------------------------- 4. blit
def oracle_blit_source(oracle, w, h, fmt):
    """a target written by row clears and a drawn frame; -> (context, the codes it holds)"""
    rng = np.random.default_rng(23 + fmt)
    rows = rng.uniform(-0.25, 1.25, (h, 4)).astype(f32)
    for y in range(0, h, 3):  # alphas 0, 1 and 2 among the seeded ones (no simple fractions: thirds of them tie at k + 1/2)
        rows[y, 3] = (0.0, 1.0, 2.0)[(y // 3) % 3]
    rows[5:7, :3] = rng.uniform(1.0, 16.0, (2, 3))  # HDR rows
    if fmt == A.COLOR_RGBA8:
        # Rows are constant, so a destination pixel between two rows is a sum of two bytes under weights of m / 128
        # (23 -> 64) or quarters: for arbitrary bytes that is exactly k + 1/2 at one pixel in 128 per channel, a whole
        # row at a time, and since an RGBA8 load is not exact every such pixel is offered.  Bytes 0 and 128 (and the
        # quads' 255) tie at weight 1/2 only.  Arbitrary bytes are the HIP library's case (a seeded tensor).
        rows = (128 * rng.integers(0, 2, (h, 4)) / 255.0).astype(f32)
    r = oracle.create(w, h, fmt)
    clear_rows(r, rows)
    quads = [IC.Layer((2, 3, w - 5, h // 2), 0.5, (128 / 255, 0.0, 1.0, 1)), IC.Layer((w // 3, h // 3, w - 2, h - 2), 0.625, (1.0, 0.0, 1.0, 1)),
             IC.Layer((1, h // 2, w // 2, h - 1), 0.75, (0.0, 1.0, 0.0, 1))]
    r.draw_geometry(IC.blend_scene(), IC.layer_objects(r, quads, w, h, transparent=False))
    codes, _ = oracle_destination(fmt, rows, quads, w, h)
    assert np.array_equal(r.read_color(), codes), "the blit's source is what S1 says the clears and the quads stored"
    return r, codes


BLIT_TOTALS = {}


@pytest.mark.parametrize("fmt", FMT_IDS)
@pytest.mark.parametrize("size", IC.BLIT_SOURCES, ids=[f"{w}x{h}" for w, h in IC.BLIT_SOURCES])
def test_blit(oracle, size, fmt):
    w, h = size
    r, codes = oracle_blit_source(oracle, w, h, IC.FORMATS[fmt])
    worst, total, offered_total = [0.0], 0, 0
    for dw, dh in IC.blit_extents(w, h):
        ref = IC.blit_reference(("oracle", w, h), codes, IC.FORMATS[fmt], dw, dh)
        for dst_format in (A.SWAPCHAIN_B8G8R8A8, A.SWAPCHAIN_R8G8B8A8):
            n, offered = IC.check_blit(f"oracle {w}x{h} {fmt} -> {dw}x{dh} format {dst_format}", r.read_swapchain(dw, dh, dst_format), ref, dst_format, worst)
        if (dw, dh) == (w, h):
            # (an RGBA8 source's load carries its two roundings, which never reach a byte's boundary: one value still)
            assert offered == 0 and (fmt == "rgba8" or all(a == 0 for a in ref.allow.reshape(-1))), "an identity extent is exact"
        total, offered_total = total + n, offered_total + offered
    r.close()
    BLIT_TOTALS[(size, fmt)] = (total, offered_total, worst[0])
    print(f"{w}x{h} {fmt}: {total} destination pixels, {offered_total} offered, worst error / allowance {worst[0]:.3f}")
    assert offered_total <= IC.EITHER_OR_CAP * total, f"{w}x{h} {fmt}: {offered_total} of {total} destination pixels offered"
    assert 0.0 < worst[0] <= 1.0


@pytest.mark.parametrize("fmt", FMT_IDS)
@pytest.mark.parametrize("size", IC.BLIT_SOURCES, ids=[f"{w}x{h}" for w, h in IC.BLIT_SOURCES])
def test_blit_either_or_cap_of_the_seeded_sources(size, fmt):
    """the HIP library's blit cases (seeded tensors): the offered share depends on the reference and the inputs alone"""
    w, h = size
    total = offered = 0
    for dw, dh in IC.blit_extents(w, h):
        key, codes = IC.blit_source_for(w, h, IC.FORMATS[fmt], dw, dh)
        ref = IC.blit_reference(key, codes, IC.FORMATS[fmt], dw, dh)
        total += dw * dh
        offered += sum(any(len(s) > 1 for s in px) for row in ref.sets for px in row)
        if (dw, dh) == (w, h):
            assert all(len(s) == 1 for s in ref.sets.reshape(-1))
        print(f"  {dw}x{dh} from {'multiples of 16' if key[3] else 'the seeded source'}: offered so far {offered}")
    print(f"seeded {w}x{h} {fmt}: {total} destination pixels, {offered} offered")
    assert offered <= IC.EITHER_OR_CAP * total


# ---------------------------------------------------------------- the reference bites
def _blend_disagrees(oracle, fmt, ks=(1, 3, 8)):
    for k in ks:
        (color, depth), codes, seed_depth, layers = oracle_blend(oracle, k, fmt)
        try:
            IC.check_blend("wrong", color, depth, codes, seed_depth, IR.blend_pass(codes, seed_depth, layers, fmt))
        except AssertionError as e:
            return f"caught: {e}"
    return None


def _store_disagrees(oracle, fmt):
    try:
        if fmt == A.COLOR_RGBA8:
            test_unorm8_store_through_row_clears(oracle)
        else:
            test_half_conversions(oracle)
    except AssertionError as e:
        return f"caught: {e}"
    return None


def _mip_disagrees(oracle):
    try:
        for content in ("random", "ties", "checker"):
            test_mip_chain(oracle, content)
    except AssertionError as e:
        return f"caught: {e}"
    return None


def _blit_disagrees(oracle):
    w, h = IC.BLIT_SOURCES[0]
    r, codes = oracle_blit_source(oracle, w, h, A.COLOR_RGBA16F)
    try:
        for dw, dh in ((w, h), (13, 7), (111, 69)):
            got = r.read_swapchain(dw, dh, A.SWAPCHAIN_B8G8R8A8)
            IC.check_blit("wrong", got, IR.blit(codes, A.COLOR_RGBA16F, dw, dh), A.SWAPCHAIN_B8G8R8A8)
    except AssertionError as e:
        return f"caught: {e}"
    finally:
        r.close()
    return None


CATCHERS = {
    "blend_src_alpha": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F), "blend_classic": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F),
    "blend_unrounded_dst": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F, (8,)), "f16_rounded_once": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F, (1,)),
    "unorm8_truncate": lambda o: _store_disagrees(o, A.COLOR_RGBA8), "unorm8_half_up": lambda o: _store_disagrees(o, A.COLOR_RGBA8),
    "depth_test_greater": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F, (3, 8)), "transparent_writes_depth": lambda o: _blend_disagrees(o, A.COLOR_RGBA16F, (8,)),
    "mip_coord_2i": _mip_disagrees, "mip_ceil_extent": _mip_disagrees, "mip_half_up": _mip_disagrees,
    "blit_taps_floor_u": _blit_disagrees, "blit_wrap": _blit_disagrees, "blit_no_swap": _blit_disagrees,
}


@pytest.mark.parametrize("variant", IR.VARIANTS)
def test_wrong_variant_of_the_reference_is_caught(oracle, variant):
    assert CATCHERS[variant](oracle) is None, "the true rules agree with the oracle on the catching cases"
    IR.WRONG = variant
    try:
        caught = CATCHERS[variant](oracle)
    finally:
        IR.WRONG = None
    print(f"{variant}: {caught}")
    assert caught, f"the reference with '{variant}' agrees with the oracle: a case is missing"
    # the RGBA8 blend as well.  (Not half-up: a sum of dyadic values times 255 is k + 1/2 only at 127.5, where half-up and
    # half-to-even agree; it takes a binary32 product that lands on k + 1/2 with k even, which the store case supplies.)
    if variant in ("unorm8_truncate", "blend_src_alpha", "blend_classic"):
        IR.WRONG = variant
        try:
            assert _blend_disagrees(oracle, A.COLOR_RGBA8), f"'{variant}' passes the RGBA8 blend cases"
        finally:
            IR.WRONG = None


if __name__ == "__main__":
    import svr_testlib
    lib = svr_testlib.load_oracle()
    for name, fmt_ in IC.FORMATS.items():
        tot = [0, 0, 0]
        for k_, s_ in BLEND_CASES:
            (c_, d_), codes_, sd_, layers_ = oracle_blend(lib, k_, fmt_, s_)
            ref_ = IR.blend_pass(codes_, sd_, layers_, fmt_, s_)
            n_, off_ = IC.check_blend("table", c_, d_, codes_, sd_, ref_)
            tot = [tot[0] + n_, tot[1] + len(ref_.sets), tot[2] + off_]
        print(f"S2 oracle {name}: {tot[0]} pixels checked, {tot[1]} blended, {tot[2]} offered")
        print(f"S2 seeded destination {name}: {[sum(v[i] for v in blend_cap_hip(fmt_).values()) for i in range(3)]} (pixels, blended, offered)")
