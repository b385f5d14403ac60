"""The upscaled present at the C boundary, without a GPU: include/svr_upscale.h against the binding and the product library's
exports, the struct layout, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_upscale.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.UPSCALE_SYMBOLS) == ["svr_read_upscaled", "svr_upscale_to_swapchain"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS, A.EXPOSURE_SYMBOLS, A.OVERLAY_SYMBOLS):
        assert not set(A.UPSCALE_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"(SVR_UPSCALE_[A-Z_]+)\s*=\s*(\d+)u?", text) == [("SVR_UPSCALE_NO_SHARPEN", str(A.UPSCALE_NO_SHARPEN))]
    assert A.UPSCALE_NO_SHARPEN == 1


def test_the_blit_keeps_its_interface():
    assert "svr_copy_to_swapchain" in A.SYMBOLS and "svr_read_swapchain" in A.SYMBOLS


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_upscale.h"
int main(void) {
  printf("SvrUpscalePass %zu\n", sizeof(SvrUpscalePass));
  printf("SvrUpscalePass.sharpness %zu\n", offsetof(SvrUpscalePass, sharpness));
  printf("SvrUpscalePass.flags %zu\n", offsetof(SvrUpscalePass, flags));
  return 0;
}
'''


def test_struct_layout_matches_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert [f for f, _ in A.SvrUpscalePass._fields_] == ["sharpness", "flags"]
    assert got == {"SvrUpscalePass": C.sizeof(A.SvrUpscalePass), "SvrUpscalePass.sharpness": A.SvrUpscalePass.sharpness.offset,
                   "SvrUpscalePass.flags": A.SvrUpscalePass.flags.offset}
    assert got == {"SvrUpscalePass": 8, "SvrUpscalePass.sharpness": 0, "SvrUpscalePass.flags": 4}


def test_header_compiles_as_c():
    src = ('#include "svr_upscale.h"\n'
           'int main(void) { int (*u)(SvrContext*, const SvrUpscalePass*, void*, uint32_t, uint32_t, int) = svr_upscale_to_swapchain;\n'
           '  int (*r)(SvrContext*, const SvrUpscalePass*, uint32_t, uint32_t, int, void*, size_t) = svr_read_upscaled;\n'
           '  SvrUpscalePass p; p.sharpness = 0.5f; p.flags = SVR_UPSCALE_NO_SHARPEN;\n'
           '  return (u == 0) + (r == 0) + (p.flags != 1u); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_upscaled_present():
    g.build()
    assert not set(A.UPSCALE_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_upscale


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.UPSCALE_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_upscale


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    p = A.SvrUpscalePass(0.5, 0)
    word = C.c_uint32(7)
    assert L.svr_upscale_to_swapchain(None, C.byref(p), C.byref(word), 4, 4, 0) == -1
    assert b"svr_upscale_to_swapchain: null" in L.svr_last_error()
    assert L.svr_upscale_to_swapchain(None, None, None, 4, 4, 0) == -1
    assert L.svr_read_upscaled(None, C.byref(p), 1, 1, 0, C.byref(word), 4) == -1
    assert b"svr_read_upscaled: null" in L.svr_last_error() and word.value == 7


@pytest.mark.parametrize("call,args", [("upscale_to_swapchain", (0, 4, 4)), ("read_upscaled", (4, 4))])
def test_oracle_is_refused_cleanly(oracle, call, args):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no upscaled present \(include/svr_upscale.h\)") as e:
        getattr(r, call)(*args)
    assert e.value.code == -5
