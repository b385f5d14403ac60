"""Multiview passes at the C boundary, without a GPU: include/svr_views.h against the binding and the product library's
exports, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_views.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.VIEWS_SYMBOLS)
    assert not set(A.VIEWS_SYMBOLS) & set(A.SYMBOLS)  # the oracle's ABI (svr.h) is unchanged
    assert "#define SVR_MAX_VIEWS 16" in open(HEADER).read() and A.MAX_VIEWS == 16


def test_product_library_exports_the_view_calls():
    g.build()
    assert not set(A.VIEWS_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_views


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.VIEWS_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_views


def test_header_compiles_as_c():
    src = ('#include "svr_views.h"\n'
           'int main(void) { SvrViewTargets t = {0, 0, 0, 0}; int (*f)(SvrContext*, SvrDrawList, uint32_t, const SvrSceneData*,\n'
           '  const SvrViewTargets*, SvrStats*) = svr_draw_list_views;\n'
           '  int (*d)(SvrContext*, uint32_t, const SvrSceneData*, const SvrViewTargets*, const SvrRenderObject*, size_t,\n'
           '  const SvrRenderObject*, size_t, SvrStats*) = svr_draw_geometry_views;\n'
           '  return (t.color != 0) + (f == 0) + (d == 0) + (SVR_MAX_VIEWS != 16); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_view_targets_layout():
    assert C.sizeof(A.SvrViewTargets) == 32
    assert [f[0] for f in A.SvrViewTargets._fields_] == ["color", "depth", "ids", "clear_rgba"]


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    t = A.SvrViewTargets()
    scenes = (A.SvrSceneData * 2)()
    assert L.svr_draw_geometry_views(None, 2, C.addressof(scenes), C.byref(t), None, 0, None, 0, None) == -1
    assert L.svr_draw_list_views(None, 1, 2, C.addressof(scenes), C.byref(t), None) == -1
    assert b"null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    for call in (lambda: r.draw_views([A.SvrSceneData()], 0, 0, None), lambda: r.draw_list_views([A.SvrSceneData()], 1, 0, 0)):
        with pytest.raises(pkg.SvrError, match="no multiview"):
            call()
