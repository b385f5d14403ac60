"""The UI overlay pass at the C boundary, without a GPU: include/svr_overlay.h against the binding and the product
library's exports, the struct layouts, the oracle's refusal, the refusals that need no device, and the built-in font."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_overlay.h")
INCLUDE = os.path.join(g.ROOT, "include")
FIELDS = {"SvrOverlayVertex": ["pos", "uv", "col"],
          "SvrOverlayCmd": ["clip_rect", "texture", "vtx_offset", "idx_offset", "elem_count"],
          "SvrOverlayTexture": ["texels", "width", "height", "format", "reserved"],
          "SvrOverlayList": ["vertices", "indices", "cmds", "textures", "n_vertices", "n_indices", "n_cmds", "n_textures", "display_pos", "scale"],
          "SvrOverlayStats": ["triangles", "kept", "tiles"]}


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.OVERLAY_SYMBOLS) == ["svr_debug_read_overlay_stats", "svr_draw_overlay", "svr_overlay_font"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS, A.EXPOSURE_SYMBOLS):
        assert not set(A.OVERLAY_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(SVR_OVERLAY_[A-Z0-9_]+)\s+(\d+)", open(HEADER).read())}
    assert defines == {"SVR_OVERLAY_MAX_TRIANGLES": A.OVERLAY_MAX_TRIANGLES, "SVR_OVERLAY_MAX_CMDS": A.OVERLAY_MAX_CMDS,
                       "SVR_OVERLAY_MAX_TEXTURES": A.OVERLAY_MAX_TEXTURES, "SVR_OVERLAY_MAX_TEXTURE_EXTENT": A.OVERLAY_MAX_TEXTURE_EXTENT,
                       "SVR_OVERLAY_TEX_RGBA8": A.OVERLAY_TEX_RGBA8, "SVR_OVERLAY_TEX_A8": A.OVERLAY_TEX_A8,
                       "SVR_OVERLAY_FONT_WHITE_X": A.OVERLAY_FONT_WHITE_X, "SVR_OVERLAY_FONT_WHITE_Y": A.OVERLAY_FONT_WHITE_Y}
    assert (A.OVERLAY_MAX_TRIANGLES, A.OVERLAY_MAX_CMDS, A.OVERLAY_MAX_TEXTURES, A.OVERLAY_MAX_TEXTURE_EXTENT) == (65536, 4096, 16, 16384)
    assert (A.OVERLAY_TEX_RGBA8, A.OVERLAY_TEX_A8) == (0, 1)


def _layout_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "svr_overlay.h"', "int main(void) {"]
    for name, fields in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_struct_layouts_match_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(_layout_source())
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for name, fields in FIELDS.items():
        cls = getattr(A, name)
        assert [f for f, _ in cls._fields_] == fields
        want[name] = C.sizeof(cls)
        for field in fields:
            want[f"{name}.{field}"] = getattr(cls, field).offset
    assert got == want
    assert (got["SvrOverlayVertex"], got["SvrOverlayCmd"], got["SvrOverlayTexture"], got["SvrOverlayStats"]) == (20, 32, 24, 12)
    assert [got[f"SvrOverlayVertex.{f}"] for f in FIELDS["SvrOverlayVertex"]] == [0, 8, 16]
    assert [got[f"SvrOverlayCmd.{f}"] for f in FIELDS["SvrOverlayCmd"]] == [0, 16, 20, 24, 28]
    assert [got[f"SvrOverlayTexture.{f}"] for f in FIELDS["SvrOverlayTexture"]] == [0, 8, 12, 16, 20]
    assert A.OVERLAY_VERTEX_DTYPE.itemsize == 20 and A.OVERLAY_CMD_DTYPE.itemsize == 32
    assert [A.OVERLAY_VERTEX_DTYPE.fields[f][1] for f in FIELDS["SvrOverlayVertex"]] == [0, 8, 16]
    assert [A.OVERLAY_CMD_DTYPE.fields[f][1] for f in FIELDS["SvrOverlayCmd"]] == [0, 16, 20, 24, 28]


def test_header_compiles_as_c():
    src = ('#include "svr_overlay.h"\n'
           'int main(void) { int (*d)(SvrContext*, void*, uint32_t, uint32_t, int, const SvrOverlayList*) = svr_draw_overlay;\n'
           '  int (*s)(SvrContext*, SvrOverlayStats*) = svr_debug_read_overlay_stats;\n'
           '  int (*f)(const uint8_t**, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*) = svr_overlay_font;\n'
           '  SvrOverlayVertex v; SvrOverlayCmd c; SvrOverlayTexture t; SvrOverlayList l; SvrOverlayStats st;\n'
           '  v.col = 0xff0000ffu; c.elem_count = 3u; t.format = SVR_OVERLAY_TEX_A8; l.n_cmds = c.elem_count / 3u; st.kept = v.col >> 31;\n'
           '  return (d == 0) + (s == 0) + (f == 0) + (t.format != 1u) + (l.n_cmds != 1u) + (st.kept != 1u) + (SVR_OVERLAY_MAX_TRIANGLES != 65536); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_overlay_pass():
    g.build()
    assert not set(A.OVERLAY_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_overlay


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.OVERLAY_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_overlay


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    lst = A.SvrOverlayList()
    assert L.svr_draw_overlay(None, C.c_void_p(64), 8, 8, 0, C.byref(lst)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_draw_overlay(None, None, 8, 8, 0, None) == -1
    st = A.SvrOverlayStats(triangles=7)
    assert L.svr_debug_read_overlay_stats(None, C.byref(st)) == -1 and st.triangles == 7
    assert b"null" in L.svr_last_error()


@pytest.mark.parametrize("call,args", [("draw_overlay", (0, 8, 8, 0, [], [], [], [])), ("read_overlay_stats", ())])
def test_oracle_is_refused_cleanly(oracle, call, args):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no overlay pass \(include/svr_overlay.h\)") as e:
        getattr(r, call)(*args)
    assert e.value.code == -5
    with pytest.raises(pkg.SvrError, match=r"has no overlay pass \(include/svr_overlay.h\)"):
        A.overlay_font(oracle)


def test_the_font_needs_no_device():
    atlas, cell_w, cell_h, first, n = A.overlay_font(pkg.load_product_library())
    assert atlas.shape == (48, 96) and atlas.dtype == np.uint8 and (cell_w, cell_h, first, n) == (6, 8, 32, 95)
    assert set(np.unique(atlas)) == {0, 255}

    def cell(ch):
        k = ch if isinstance(ch, int) else ord(ch) - first
        return atlas[(k // 16) * 8:(k // 16) * 8 + 8, (k % 16) * 6:(k % 16) * 6 + 6]

    digits = [cell(d).tobytes() for d in "0123456789"]
    assert len(set(digits)) == 10
    assert not cell(" ").any()
    for ch in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ.,:-+%/()_":
        assert cell(ch).any() and not cell(ch)[:, 5].any() and not cell(ch)[7].any(), ch  # 5 x 7 in the cell's top left
        assert not cell(ch)[:7, :5].all(), ch  # a drawn glyph, not the box
    letters = [cell(c).tobytes() for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ"]
    assert len(set(letters)) == 26
    for lower, upper in zip("abcxyz", "ABCXYZ"):
        assert np.array_equal(cell(lower), cell(upper))
    assert cell("#")[:7, :5].all() and cell("~")[:7, :5].all()  # anything else: a filled box
    # the opaque texel and its neighbours, so that a bilinear tap at its centre is exactly 1
    x, y = A.OVERLAY_FONT_WHITE_X, A.OVERLAY_FONT_WHITE_Y
    assert (atlas[y - 1:y + 2, x - 1:x + 2] == 255).all() and cell(95).all()
    # null outputs are allowed
    L = pkg.load_product_library().lib
    assert L.svr_overlay_font(None, None, None, None, None, None, None) == 0


def test_the_list_builder_makes_a_window():
    font = A.overlay_font(pkg.load_product_library())
    b = pkg.overlay.ListBuilder(font)
    b.window(4, 6, 100, 40, "stats")
    b.text(8, 20, "draws 12", (255, 255, 255, 255))
    b.rect(8, 30, 10, 4, (255, 0, 0, 128))
    vertices, indices, cmds = b.arrays()
    quads = 2 + 5 + 7 + 1  # body, bar, "stats", "draws 12" without its space, the rectangle
    assert vertices.size == 4 * quads and indices.size == 6 * quads and indices.dtype == np.uint16 and int(indices.max()) == vertices.size - 1
    assert cmds.size == 1 and tuple(cmds[0]["clip_rect"]) == (4.0, 6.0, 104.0, 46.0) and cmds[0]["elem_count"] == 6 * quads
    assert vertices[-1]["col"] == 0x800000ff
    b.window(50, 50, 20, 20, "b")
    _, _, cmds = b.arrays()
    assert cmds.size == 2 and cmds[1]["vtx_offset"] == 4 * quads and cmds[1]["idx_offset"] == 6 * quads
