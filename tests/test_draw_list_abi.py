"""Retained draw lists at the C boundary, without a GPU: include/svr_draw_list.h against the binding and the product
library's exports, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_draw_list.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.DRAW_LIST_SYMBOLS)
    assert not set(A.DRAW_LIST_SYMBOLS) & set(A.SYMBOLS)  # the oracle's ABI (svr.h) is unchanged


def test_product_library_exports_the_draw_list_calls():
    g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.PRODUCT_LIBRARY], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not set(A.DRAW_LIST_SYMBOLS) - exported
    assert pkg.load_product_library().has_draw_lists


def test_header_compiles_as_c():
    src = '#include "svr_draw_list.h"\nint main(void) { SvrDrawList l = 0; return (int)l + (int)sizeof(SvrRenderObject) - 108; }\n'
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_record_sizes_match_the_device_structs():
    text = open(os.path.join(g.PKG_DIR, "csrc", "svr_device.h")).read()
    assert f"sizeof(DrawDesc) == {A.DRAW_DESC_BYTES}" in text
    assert "uint32_t draw;\n  uint32_t first_tri;" in text and A.WAVE_CHUNK_BYTES == 8


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    out = C.c_uint32()
    obj = A.SvrRenderObject()
    scene = A.SvrSceneData()
    st = A.SvrStats()
    assert L.svr_create_draw_list(None, None, 0, None, 0, C.byref(out)) == -1
    assert L.svr_update_draw_list(None, 1, 0, C.byref(obj), 1) == -1
    assert L.svr_draw_list(None, 1, C.byref(scene), C.byref(st)) == -1
    assert L.svr_destroy_draw_list(None, 1) == -4
    assert L.svr_debug_read_records(None, None, 0, None, 0, None, None) == -1
    assert b"null" in L.svr_last_error()


def test_oracle_has_no_draw_lists(oracle):
    assert not oracle.has_draw_lists
    r = pkg.abi.Renderer.__new__(pkg.abi.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match="no draw lists"):
        r.create_draw_list(None)
