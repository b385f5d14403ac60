"""The reflection pass at the C boundary, without a GPU: include/svr_reflect.h against the binding and the product
library's exports, the struct layout, the oracle's refusal, and the refusals that need no device.  (The refusals that need
a context, and that they leave the targets' bits alone, are in test_reflect_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_reflect.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.REFLECT_SYMBOLS) == ["svr_reflect_pass"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS, A.EXPOSURE_SYMBOLS,
                  A.OVERLAY_SYMBOLS, A.UPSCALE_SYMBOLS, A.FOG_SYMBOLS, A.DOF_SYMBOLS, A.MOTION_SYMBOLS):
        assert not set(A.REFLECT_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = open(HEADER).read()
    steps, refine = (re.search(rf"#define\s+{name}\s+(\d+)", text) for name in ("SVR_REFLECT_MAX_STEPS", "SVR_REFLECT_MAX_REFINE"))
    assert steps and int(steps.group(1)) == A.REFLECT_MAX_STEPS == 64
    assert refine and int(refine.group(1)) == A.REFLECT_MAX_REFINE == 8


def test_header_has_the_sections_and_states_what_is_out_of_scope():
    text = " ".join(open(HEADER).read().split())
    heads = ["In place on the context's colour target", "Arithmetic (DESIGN.md §3, C73-C79)", "Refusals, with nothing changed", "Ordering", "Out of scope"]
    assert [text.index(s) for s in heads] == sorted(text.index(s) for s in heads)
    scope = text[text.index("Out of scope"):]
    for phrase in ("oracle", "Multiview layers", "sharded frame", "depth hierarchy", "farthest depth", "linear march with a bisection refinement",
                   "roughness", "back faces", "off screen or behind the visible surface"):
        assert phrase in scope, phrase


FIELDS = [f for f, _ in A.SvrReflectPass._fields_]
LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_reflect.h"
#define F(f) printf("SvrReflectPass." #f " %zu\n", offsetof(SvrReflectPass, f));
int main(void) {
  printf("SvrReflectPass %zu\n", sizeof(SvrReflectPass));
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
    want = {"SvrReflectPass": C.sizeof(A.SvrReflectPass)}
    for field in FIELDS:
        want[f"SvrReflectPass.{field}"] = getattr(A.SvrReflectPass, field).offset
    assert got == want
    assert got["SvrReflectPass"] == 192
    assert [got[f"SvrReflectPass.{f}"] for f in FIELDS] == [0, 64, 128, 140, 144, 148, 152, 156, 160, 164, 168, 172, 176, 180, 184, 188]
    # every field the header declares is bound, in order
    body = re.search(r"typedef struct SvrReflectPass \{(.*?)\} SvrReflectPass;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == FIELDS


def test_header_compiles_as_c():
    src = ('#include "svr_reflect.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrReflectPass*) = svr_reflect_pass;\n'
           '  SvrReflectPass p; p.steps = SVR_REFLECT_MAX_STEPS; p.refine = SVR_REFLECT_MAX_REFINE; p.viewproj[15] = 1;\n'
           '  return (f == 0) + (p.steps != 64) + (p.refine != 8) + (p.viewproj[15] != 1); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_reflection_pass():
    g.build()
    assert not set(A.REFLECT_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_reflect


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.REFLECT_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_reflect


def test_product_never_links_the_oracle():
    g.build()
    out = subprocess.run(["readelf", "-d", pkg.PRODUCT_LIBRARY], check=True, stdout=subprocess.PIPE, text=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", out)
    assert needed and not [n for n in needed if "oracle" in n], needed


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    I = pkg.glmath.identity()
    p = A.reflect_struct(I, I, (0.0, 0.0, 0.0), 1.0, 0.0)
    assert L.svr_reflect_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_reflect_pass(None, None) == -1


def test_reflect_struct_fills_every_field():
    m = [[float(4 * c + r) for r in range(4)] for c in range(4)]  # [col][row]: column-major in memory
    inv = [[float(100 + 4 * c + r) for r in range(4)] for c in range(4)]
    p = A.reflect_struct(m, inv, (1.0, 2.0, 3.0), 0.5, 0.25, max_distance=7.0, steps=9, refine=3, thickness=0.125, f0=0.75, intensity=2.0,
                         distance_fade=0.375, edge_width=5.0, resolve=0, depth_tolerance=0.0625, frame_index=-1)
    assert list(p.viewproj) == [float(i) for i in range(16)] and list(p.inv_viewproj) == [float(100 + i) for i in range(16)]
    assert list(p.camera_position) == [1.0, 2.0, 3.0]
    assert (p.inv_z_scale, p.inv_z_bias, p.max_distance, p.steps, p.refine) == (0.5, 0.25, 7.0, 9, 3)
    assert (p.thickness, p.f0, p.intensity, p.distance_fade, p.edge_width, p.resolve, p.depth_tolerance) == (0.125, 0.75, 2.0, 0.375, 5.0, 0, 0.0625)
    assert p.frame_index == 0xffffffff
    d = A.reflect_struct(m, inv, (0.0, 0.0, 0.0), 1.0, 0.0)
    assert (d.steps, d.refine, d.resolve) == (16, 4, 1)


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    I = pkg.glmath.identity()
    with pytest.raises(pkg.SvrError, match=r"has no reflection pass \(include/svr_reflect.h\)") as e:
        r.reflect_pass(I, I, (0.0, 0.0, 0.0), 1.0, 0.0)
    assert e.value.code == -5
