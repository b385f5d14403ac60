"""Depth-only passes at the C boundary, without a GPU: include/svr_depth.h against the binding and the product library's
exports, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_depth.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.DEPTH_SYMBOLS)
    assert not set(A.DEPTH_SYMBOLS) & set(A.SYMBOLS)  # the oracle's ABI (svr.h) is unchanged
    assert not set(A.DEPTH_SYMBOLS) & set(A.VIEWS_SYMBOLS + A.DRAW_LIST_SYMBOLS + A.ID_SYMBOLS)


def test_product_library_exports_the_depth_calls():
    g.build()
    assert not set(A.DEPTH_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_depth


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.DEPTH_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_depth


def test_header_compiles_as_c():
    src = ('#include "svr_depth.h"\n'
           'int main(void) {\n'
           '  int (*a)(SvrContext*, const SvrSceneData*, const SvrRenderObject*, size_t, SvrStats*) = svr_draw_depth;\n'
           '  int (*b)(SvrContext*, SvrDrawList, const SvrSceneData*, SvrStats*) = svr_draw_list_depth;\n'
           '  int (*c)(SvrContext*, uint32_t, const SvrSceneData*, const SvrViewTargets*, const SvrRenderObject*, size_t,\n'
           '           SvrStats*) = svr_draw_depth_views;\n'
           '  int (*d)(SvrContext*, SvrDrawList, uint32_t, const SvrSceneData*, const SvrViewTargets*, SvrStats*) =\n'
           '      svr_draw_list_depth_views;\n'
           '  return (a == 0) + (b == 0) + (c == 0) + (d == 0); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_makefile_tracks_the_header():
    mk = open(os.path.join(g.PKG_DIR, "csrc", "Makefile")).read()
    assert "../../include/svr_depth.h" in mk


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    t = A.SvrViewTargets()
    scene = A.SvrSceneData()
    scenes = (A.SvrSceneData * 2)()
    assert L.svr_draw_depth(None, C.byref(scene), None, 0, None) == -1
    assert b"svr_draw_depth: null" in L.svr_last_error()
    assert L.svr_draw_list_depth(None, 1, C.byref(scene), None) == -1
    assert b"svr_draw_list_depth: null" in L.svr_last_error()
    assert L.svr_draw_depth_views(None, 2, C.addressof(scenes), C.byref(t), None, 0, None) == -1
    assert b"svr_draw_depth_views: null" in L.svr_last_error()
    assert L.svr_draw_list_depth_views(None, 1, 2, C.addressof(scenes), C.byref(t), None) == -1
    assert b"svr_draw_list_depth_views: null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    for call in (lambda: r.draw_depth(A.SvrSceneData(), None), lambda: r.draw_list_depth(A.SvrSceneData(), 1),
                 lambda: r.draw_depth_views([A.SvrSceneData()], 0, None), lambda: r.draw_list_depth_views([A.SvrSceneData()], 1, 0)):
        with pytest.raises(pkg.SvrError, match="no depth-only"):
            call()
