"""The camera motion blur pass at the C boundary, without a GPU: include/svr_motion.h against the binding and the product
library's exports, the struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_motion.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.MOTION_SYMBOLS) == ["svr_motion_blur_pass"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS, A.EXPOSURE_SYMBOLS,
                  A.OVERLAY_SYMBOLS, A.UPSCALE_SYMBOLS, A.FOG_SYMBOLS, A.DOF_SYMBOLS):
        assert not set(A.MOTION_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    m = re.search(r"#define\s+SVR_MOTION_MAX_BLUR\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == A.MOTION_MAX_BLUR == 16


def test_header_has_the_sections_and_states_what_is_out_of_scope():
    text = " ".join(open(HEADER).read().split())
    heads = ["In place on the context's colour target", "Arithmetic (DESIGN.md §3, C67-C72)", "Refusals, with nothing changed", "Ordering", "Out of scope"]
    assert [text.index(s) for s in heads] == sorted(text.index(s) for s in heads)
    scope = text[text.index("Out of scope"):]
    for phrase in ("oracle", "Multiview layers", "sharded frame", "Per-object motion", "Per-pixel dither", "A direction per tap"):
        assert phrase in scope, phrase


FIELDS = [f for f, _ in A.SvrMotionBlurPass._fields_]
LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_motion.h"
#define F(f) printf("SvrMotionBlurPass." #f " %zu\n", offsetof(SvrMotionBlurPass, f));
int main(void) {
  printf("SvrMotionBlurPass %zu\n", sizeof(SvrMotionBlurPass));
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
    want = {"SvrMotionBlurPass": C.sizeof(A.SvrMotionBlurPass)}
    for field in FIELDS:
        want[f"SvrMotionBlurPass.{field}"] = getattr(A.SvrMotionBlurPass, field).offset
    assert got == want
    assert got["SvrMotionBlurPass"] == 72
    assert [got[f"SvrMotionBlurPass.{f}"] for f in FIELDS] == [0, 64, 68]
    # every field the header declares is bound, in order
    body = re.search(r"typedef struct SvrMotionBlurPass \{(.*?)\} SvrMotionBlurPass;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == FIELDS


def test_header_compiles_as_c():
    src = ('#include "svr_motion.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrMotionBlurPass*) = svr_motion_blur_pass;\n'
           '  SvrMotionBlurPass p; p.max_blur = SVR_MOTION_MAX_BLUR; p.shutter = 0; p.reproject[15] = 1;\n'
           '  return (f == 0) + (p.max_blur != 16) + (p.shutter != 0) + (p.reproject[15] != 1); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_motion_blur_pass():
    g.build()
    assert not set(A.MOTION_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_motion


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.MOTION_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_motion


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.motion_struct(pkg.glmath.identity(), 1.0)
    assert L.svr_motion_blur_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_motion_blur_pass(None, None) == -1


def test_motion_struct_fills_every_field():
    m = [[float(4 * c + r) for r in range(4)] for c in range(4)]  # [col][row]: column-major in memory
    p = A.motion_struct(m, 0.5, 12.0)
    assert list(p.reproject) == [float(i) for i in range(16)] and (p.shutter, p.max_blur) == (0.5, 12.0)
    assert A.motion_struct(m, 1.0).max_blur == A.MOTION_MAX_BLUR


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no motion blur pass \(include/svr_motion.h\)") as e:
        r.motion_blur_pass(pkg.glmath.identity(), 1.0)
    assert e.value.code == -5
