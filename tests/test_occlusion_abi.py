"""Occlusion culling at the C boundary, without a GPU: include/svr_occlusion.h against the binding and the product
library's exports, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_occlusion.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.OCCLUSION_SYMBOLS)
    others = A.SYMBOLS + A.DRAW_LIST_SYMBOLS + A.ID_SYMBOLS + A.VIEWS_SYMBOLS + A.DEPTH_SYMBOLS
    assert not set(A.OCCLUSION_SYMBOLS) & set(others)


def test_product_library_exports_the_occlusion_calls():
    g.build()
    assert not set(A.OCCLUSION_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_occlusion


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.OCCLUSION_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_occlusion


def test_header_compiles_as_c():
    src = ('#include "svr_occlusion.h"\n'
           'int main(void) {\n'
           '  int (*a)(SvrContext*, SvrDepthPyramid*) = svr_create_depth_pyramid;\n'
           '  int (*b)(SvrContext*, SvrDepthPyramid) = svr_destroy_depth_pyramid;\n'
           '  int (*c)(SvrContext*, SvrDepthPyramid, const float*) = svr_build_depth_pyramid;\n'
           '  int (*d)(SvrContext*, SvrDepthPyramid) = svr_set_occlusion_pyramid;\n'
           '  int (*e)(SvrContext*, SvrDepthPyramid, uint32_t, void*, size_t, uint32_t*) = svr_read_depth_pyramid;\n'
           '  int (*f)(SvrContext*, SvrOcclusionStats*) = svr_get_occlusion_stats;\n'
           '  int (*h)(SvrContext*, uint32_t*, size_t, uint32_t*) = svr_debug_read_occlusion;\n'
           '  return (a == 0) + (b == 0) + (c == 0) + (d == 0) + (e == 0) + (f == 0) + (h == 0); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_stats_struct_layout():
    assert C.sizeof(A.SvrOcclusionStats) == 24
    assert [f for f, _ in A.SvrOcclusionStats._fields_] == ["chunks_tested", "chunks_culled", "triangles_culled"]


def test_makefile_tracks_the_header_and_the_kernel():
    mk = open(os.path.join(g.PKG_DIR, "csrc", "Makefile")).read()
    assert "../../include/svr_occlusion.h" in mk and "k_pyramid.hip" in mk


def test_refusals_without_a_device():
    L = pkg.load_product_library().lib
    h = C.c_uint32(0)
    st = A.SvrOcclusionStats()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.svr_create_depth_pyramid(None, C.byref(h)) == -1
    assert b"svr_create_depth_pyramid: null" in L.svr_last_error()
    assert L.svr_destroy_depth_pyramid(None, 1) == -1
    assert L.svr_build_depth_pyramid(None, 1, None) == -1
    assert L.svr_set_occlusion_pyramid(None, 0) == -1
    assert L.svr_read_depth_pyramid(None, 1, 1, buf, 16, None) == -1
    assert L.svr_get_occlusion_stats(None, C.byref(st)) == -1
    assert b"svr_get_occlusion_stats: null" in L.svr_last_error()
    assert L.svr_debug_read_occlusion(None, buf, 4, C.byref(n)) == -1
    assert b"svr_debug_read_occlusion: null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    for call in (r.create_depth_pyramid, lambda: r.build_depth_pyramid(1), lambda: r.set_occlusion_pyramid(0),
                 lambda: r.read_depth_pyramid(1, 1), r.occlusion_stats, r.read_occlusion, lambda: r.destroy_depth_pyramid(1)):
        with pytest.raises(pkg.SvrError, match="no occlusion culling"):
            call()
