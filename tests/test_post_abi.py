"""The HDR post pass at the C boundary, without a GPU: include/svr_post.h against the binding and the product library's
exports, the struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_post.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.POST_SYMBOLS) == ["svr_post_pass"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS):
        assert not set(A.POST_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = open(HEADER).read()
    m = re.search(r"#define\s+SVR_POST_MAX_LEVELS\s+(\d+)", text)
    assert m and int(m.group(1)) == A.POST_MAX_LEVELS == 8
    names = dict(re.findall(r"(SVR_TONEMAP_[A-Z]+)\s*=\s*(\d+)", text))
    assert {k: int(v) for k, v in names.items()} == {"SVR_TONEMAP_CLAMP": A.TONEMAP_CLAMP, "SVR_TONEMAP_REINHARD": A.TONEMAP_REINHARD,
                                                     "SVR_TONEMAP_ACES": A.TONEMAP_ACES}
    assert (A.TONEMAP_CLAMP, A.TONEMAP_REINHARD, A.TONEMAP_ACES) == (0, 1, 2)


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_post.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("SvrPostPass %zu\n", sizeof(SvrPostPass));
  F(SvrPostPass, exposure); F(SvrPostPass, bloom_threshold); F(SvrPostPass, bloom_intensity); F(SvrPostPass, bloom_levels);
  F(SvrPostPass, tonemap);
  return 0;
}
'''


def test_struct_layout_matches_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {"SvrPostPass": C.sizeof(A.SvrPostPass)}
    for field, _ in A.SvrPostPass._fields_:
        want[f"SvrPostPass.{field}"] = getattr(A.SvrPostPass, field).offset
    assert got == want
    assert got["SvrPostPass"] == 20
    assert [got[f"SvrPostPass.{f}"] for f, _ in A.SvrPostPass._fields_] == [0, 4, 8, 12, 16]


def test_header_compiles_as_c():
    src = ('#include "svr_post.h"\n'
           'int main(void) { int (*f)(SvrContext*, const SvrPostPass*) = svr_post_pass;\n'
           '  SvrPostPass p; p.bloom_levels = SVR_POST_MAX_LEVELS; p.tonemap = SVR_TONEMAP_ACES;\n'
           '  return (f == 0) + (p.bloom_levels != 8) + (p.tonemap != 2); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_post_pass():
    g.build()
    assert not set(A.POST_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_post


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.POST_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_post


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.SvrPostPass(1.0, 1.0, 1.0, 4, A.TONEMAP_ACES)
    assert L.svr_post_pass(None, C.byref(p)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_post_pass(None, None) == -1


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no post pass \(include/svr_post.h\)") as e:
        r.post_pass()
    assert e.value.code == -5
