"""The ambient pass at the C boundary, without a GPU: include/svr_ambient.h against the binding and the product library's
exports, the struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_ambient.h")
INCLUDE = os.path.join(g.ROOT, "include")
FIELDS = ["inv_viewproj", "radius", "pixels_per_unit", "bias", "intensity", "sharpness", "flags"]


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.AMBIENT_SYMBOLS) == [
        "svr_ambient_pass", "svr_bind_ambient_target", "svr_debug_read_ambient_raw", "svr_get_ambient_target", "svr_read_ambient",
        "svr_set_light_ambient_occlusion"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS):
        assert not set(A.AMBIENT_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = open(HEADER).read()
    assert dict(re.findall(r"(SVR_AMBIENT_NO_BLUR)\s*=\s*(\d+)u", text)) == {"SVR_AMBIENT_NO_BLUR": str(A.AMBIENT_NO_BLUR)}
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(SVR_AMBIENT_[A-Z_]+)\s+(\d+)", text)}
    assert defines == {"SVR_AMBIENT_MAX_REACH": A.AMBIENT_MAX_REACH, "SVR_AMBIENT_TAPS": A.AMBIENT_TAPS}
    assert (A.AMBIENT_NO_BLUR, A.AMBIENT_MAX_REACH, A.AMBIENT_TAPS) == (1, 16, 8)


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_ambient.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("SvrAmbientPass %zu\n", sizeof(SvrAmbientPass));
  F(SvrAmbientPass, inv_viewproj); F(SvrAmbientPass, radius); F(SvrAmbientPass, pixels_per_unit); F(SvrAmbientPass, bias);
  F(SvrAmbientPass, intensity); F(SvrAmbientPass, sharpness); F(SvrAmbientPass, flags);
  return 0;
}
'''


def test_struct_layout_matches_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert [f for f, _ in A.SvrAmbientPass._fields_] == FIELDS
    want = {"SvrAmbientPass": C.sizeof(A.SvrAmbientPass)}
    for field in FIELDS:
        want[f"SvrAmbientPass.{field}"] = getattr(A.SvrAmbientPass, field).offset
    assert got == want
    assert got["SvrAmbientPass"] == 88
    assert [got[f"SvrAmbientPass.{f}"] for f in FIELDS] == [0, 64, 68, 72, 76, 80, 84]


def test_header_compiles_as_c():
    src = ('#include "svr_ambient.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrAmbientPass*) = svr_ambient_pass;\n'
           '  int (*b)(SvrContext*, float*) = svr_bind_ambient_target;\n'
           '  int (*t)(SvrContext*, float**) = svr_get_ambient_target;\n'
           '  int (*r)(SvrContext*, void*, size_t) = svr_read_ambient;\n'
           '  int (*s)(SvrContext*, int) = svr_set_light_ambient_occlusion;\n'
           '  int (*d)(SvrContext*, void*, size_t) = svr_debug_read_ambient_raw;\n'
           '  SvrAmbientPass p; p.flags = SVR_AMBIENT_NO_BLUR; p.radius = 0.5f; p.inv_viewproj[15] = 1.0f;\n'
           '  return (f == 0) + (b == 0) + (t == 0) + (r == 0) + (s == 0) + (d == 0) + (p.flags != 1u) + (SVR_AMBIENT_MAX_REACH != 2 * SVR_AMBIENT_TAPS); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_ambient_pass():
    g.build()
    assert not set(A.AMBIENT_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_ambient


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.AMBIENT_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_ambient


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.SvrAmbientPass()
    p.inv_viewproj[0] = p.inv_viewproj[5] = p.inv_viewproj[10] = p.inv_viewproj[15] = 1.0
    p.radius, p.pixels_per_unit = 0.5, 100.0
    assert L.svr_ambient_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_ambient_pass(None, None) == -1
    buf = (C.c_float * 4)()
    target = C.c_void_p(7)
    assert L.svr_bind_ambient_target(None, None) == -1
    assert L.svr_get_ambient_target(None, C.byref(target)) == -1 and target.value == 7
    assert L.svr_read_ambient(None, buf, 16) == -1
    assert L.svr_debug_read_ambient_raw(None, buf, 16) == -1
    assert L.svr_set_light_ambient_occlusion(None, 1) == -1
    assert b"null" in L.svr_last_error()


@pytest.mark.parametrize("call", ["ambient_pass", "bind_ambient_target", "read_ambient", "read_ambient_raw", "set_light_ambient_occlusion"])
def test_oracle_is_refused_cleanly(oracle, call):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no ambient pass \(include/svr_ambient.h\)") as e:
        if call == "ambient_pass":
            r.ambient_pass([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], 0.5, 100.0)
        elif call == "bind_ambient_target":
            r.bind_ambient_target(None)
        else:
            getattr(r, call)()
    assert e.value.code == -5
