"""The deferred lighting pass at the C boundary, without a GPU: include/svr_lighting.h against the binding and the product
library's exports, the struct layouts, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_lighting.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.LIGHTING_SYMBOLS)
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS):
        assert not set(A.LIGHTING_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    m = re.search(r"#define\s+SVR_MAX_LIGHTS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == A.MAX_LIGHTS == 4096


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_lighting.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("SvrPointLight %zu\nSvrLightPass %zu\n", sizeof(SvrPointLight), sizeof(SvrLightPass));
  F(SvrPointLight, position); F(SvrPointLight, radius); F(SvrPointLight, color); F(SvrPointLight, intensity);
  F(SvrLightPass, inv_viewproj); F(SvrLightPass, ambient_color); F(SvrLightPass, sunlight_direction); F(SvrLightPass, sunlight_color);
  F(SvrLightPass, lights); F(SvrLightPass, n_lights); F(SvrLightPass, shadow_depth); F(SvrLightPass, shadow_width);
  F(SvrLightPass, shadow_height); F(SvrLightPass, shadow_viewproj); F(SvrLightPass, shadow_bias);
  return 0;
}
'''


def test_struct_layouts_match_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {"SvrPointLight": C.sizeof(A.SvrPointLight), "SvrLightPass": C.sizeof(A.SvrLightPass)}
    for name, T in (("SvrPointLight", A.SvrPointLight), ("SvrLightPass", A.SvrLightPass)):
        for field, _ in T._fields_:
            want[f"{name}.{field}"] = getattr(T, field).offset
    assert got == want
    assert got["SvrPointLight"] == 32 == A.POINT_LIGHT_DTYPE.itemsize
    for field, _ in A.SvrPointLight._fields_:
        assert A.POINT_LIGHT_DTYPE.fields[field][1] == getattr(A.SvrPointLight, field).offset


def test_header_compiles_as_c():
    src = ('#include "svr_lighting.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrLightPass*) = svr_light_pass;\n'
           '  int (*t)(SvrContext*, uint32_t*, size_t, uint32_t*) = svr_debug_read_light_tiles;\n'
           '  SvrLightPass p; p.n_lights = SVR_MAX_LIGHTS; return (f == 0) + (t == 0) + (p.n_lights != 4096); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_lighting_calls():
    g.build()
    assert not set(A.LIGHTING_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_lighting


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.LIGHTING_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_lighting


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.SvrLightPass()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.svr_light_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_light_pass(None, None) == -1
    assert L.svr_debug_read_light_tiles(None, buf, 4, C.byref(n)) == -1
    assert b"null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    ident = np.eye(4, dtype=np.float32)
    for call in (lambda: r.light_pass(ident, (0.1,) * 4, (0, 1, 0, 1), (1,) * 4), lambda: r.read_light_tiles()):
        with pytest.raises(pkg.SvrError, match="no lighting pass") as e:
            call()
        assert e.value.code == -5
