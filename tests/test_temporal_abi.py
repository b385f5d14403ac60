"""Temporal antialiasing at the C boundary, without a GPU: include/svr_temporal.h against the binding and the product
library's exports, the struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_temporal.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.TEMPORAL_SYMBOLS) == ["svr_debug_read_temporal_history", "svr_temporal_resolve"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS):
        assert not set(A.TEMPORAL_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = open(HEADER).read()
    names = dict(re.findall(r"(SVR_TEMPORAL_[A-Z_]+)\s*=\s*(\d+)u", text))
    assert {k: int(v) for k, v in names.items()} == {"SVR_TEMPORAL_RESET": A.TEMPORAL_RESET, "SVR_TEMPORAL_NO_CLAMP": A.TEMPORAL_NO_CLAMP}
    assert (A.TEMPORAL_RESET, A.TEMPORAL_NO_CLAMP) == (1, 2)


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_temporal.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("SvrTemporalPass %zu\n", sizeof(SvrTemporalPass));
  F(SvrTemporalPass, reproject); F(SvrTemporalPass, blend); F(SvrTemporalPass, flags);
  return 0;
}
'''


def test_struct_layout_matches_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {"SvrTemporalPass": C.sizeof(A.SvrTemporalPass)}
    for field, _ in A.SvrTemporalPass._fields_:
        want[f"SvrTemporalPass.{field}"] = getattr(A.SvrTemporalPass, field).offset
    assert got == want
    assert got["SvrTemporalPass"] == 72
    assert [got[f"SvrTemporalPass.{f}"] for f, _ in A.SvrTemporalPass._fields_] == [0, 64, 68]


def test_header_compiles_as_c():
    src = ('#include "svr_temporal.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrTemporalPass*) = svr_temporal_resolve;\n'
           '  int (*h)(SvrContext*, void*, size_t, uint32_t*) = svr_debug_read_temporal_history;\n'
           '  SvrTemporalPass p; p.flags = SVR_TEMPORAL_RESET | SVR_TEMPORAL_NO_CLAMP; p.blend = 0.1f; p.reproject[15] = 1.0f;\n'
           '  return (f == 0) + (h == 0) + (p.flags != 3u); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_temporal_pass():
    g.build()
    assert not set(A.TEMPORAL_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_temporal


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.TEMPORAL_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_temporal


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.SvrTemporalPass()
    p.reproject[0] = p.reproject[5] = p.reproject[10] = p.reproject[15] = 1.0
    p.blend = 0.1
    assert L.svr_temporal_resolve(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_temporal_resolve(None, None) == -1
    valid = C.c_uint32(7)
    assert L.svr_debug_read_temporal_history(None, None, 0, C.byref(valid)) == -1
    assert b"null" in L.svr_last_error() and valid.value == 7


@pytest.mark.parametrize("call", ["temporal_resolve", "read_temporal_history"])
def test_oracle_is_refused_cleanly(oracle, call):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no temporal pass \(include/svr_temporal.h\)") as e:
        if call == "temporal_resolve":
            r.temporal_resolve([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], 0.1)
        else:
            r.read_temporal_history()
    assert e.value.code == -5
