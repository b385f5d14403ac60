"""The fog pass at the C boundary, without a GPU: include/svr_fog.h against the binding and the product library's exports, the
struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_fog.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.FOG_SYMBOLS) == ["svr_fog_pass"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS, A.EXPOSURE_SYMBOLS,
                  A.OVERLAY_SYMBOLS, A.UPSCALE_SYMBOLS):
        assert not set(A.FOG_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    m = re.search(r"#define\s+SVR_FOG_MAX_STEPS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == A.FOG_MAX_STEPS == 64


def test_header_states_what_is_out_of_scope():
    text = " ".join(open(HEADER).read().split())
    scope = text[text.index("Out of scope"):]
    for phrase in ("oracle", "Point lights", "sharded frame", "Cascades or filtered shadows"):
        assert phrase in scope, phrase


FIELDS = [f for f, _ in A.SvrFogPass._fields_]
LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_fog.h"
#define F(f) printf("SvrFogPass." #f " %zu\n", offsetof(SvrFogPass, f));
int main(void) {
  printf("SvrFogPass %zu\n", sizeof(SvrFogPass));
  FIELD_LINES
  return 0;
}
'''.replace("FIELD_LINES", " ".join(f"F({f})" for f in FIELDS))


def test_struct_layout_matches_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {"SvrFogPass": C.sizeof(A.SvrFogPass)}
    for field in FIELDS:
        want[f"SvrFogPass.{field}"] = getattr(A.SvrFogPass, field).offset
    assert got == want
    assert got["SvrFogPass"] == 232
    assert [got[f"SvrFogPass.{f}"] for f in FIELDS] == [0, 64, 76, 80, 84, 88, 92, 96, 108, 112, 128, 140, 144, 152, 156, 160, 224, 228]
    # every field the header declares is bound, in order
    body = re.search(r"typedef struct SvrFogPass \{(.*?)\} SvrFogPass;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == FIELDS


def test_header_compiles_as_c():
    src = ('#include "svr_fog.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrFogPass*) = svr_fog_pass;\n'
           '  SvrFogPass p; p.steps = SVR_FOG_MAX_STEPS; p.shadow_depth = 0;\n'
           '  return (f == 0) + (p.steps != 64) + (p.shadow_depth != 0); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_fog_pass():
    g.build()
    assert not set(A.FOG_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_fog


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.FOG_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_fog


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.fog_struct([1.0] * 16, (0.0, 0.0, 0.0), 0.1)
    assert L.svr_fog_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_fog_pass(None, None) == -1


def test_fog_struct_fills_every_field():
    p = A.fog_struct(range(16), (1, 2, 3), 0.25, 0.5, -1.0, 80.0, 9, (0.1, 0.2, 0.3), (0, 1, 0), (4, 5, 6), -0.3, shadow_ptr=4096,
                     shadow_size=(8, 4), shadow_viewproj=range(16, 32), shadow_bias=0.01, edge_sharpness=3.0, frame_index=(1 << 32) + 7)
    assert list(p.inv_viewproj) == list(range(16)) and list(p.camera_position) == [1, 2, 3]
    assert (p.density, p.height_falloff, p.height_base, p.max_distance, p.steps) == (0.25, 0.5, -1.0, 80.0, 9)
    assert list(p.sunlight_direction) == [0, 1, 0, 0] and list(p.sun_color) == [4, 5, 6]
    assert p.shadow_depth == 4096 and (p.shadow_width, p.shadow_height) == (8, 4) and list(p.shadow_viewproj) == list(range(16, 32))
    assert p.edge_sharpness == 3.0 and p.frame_index == 7


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no fog pass \(include/svr_fog.h\)") as e:
        r.fog_pass([1.0] * 16, (0, 0, 0), 0.1)
    assert e.value.code == -5
