"""Attribute targets at the C boundary, without a GPU: include/svr_attributes.h against the binding and the product
library's exports, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_attributes.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.ATTRIBUTE_SYMBOLS)
    assert not set(A.ATTRIBUTE_SYMBOLS) & set(A.SYMBOLS)  # the oracle's ABI (svr.h) is unchanged
    for other in (A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS):
        assert not set(A.ATTRIBUTE_SYMBOLS) & set(other)


def test_header_constants_match_binding():
    text = open(HEADER).read()
    for name, value in (("BARY", A.ATTR_BARY), ("UV", A.ATTR_UV), ("NORMAL", A.ATTR_NORMAL), ("ALBEDO", A.ATTR_ALBEDO),
                        ("ALL", A.ATTR_ALL)):
        m = re.search(r"\bSVR_ATTR_%s\s*=\s*(\d+)" % name, text)
        assert m and int(m.group(1)) == value, name
    assert (A.ATTR_BARY, A.ATTR_UV, A.ATTR_NORMAL, A.ATTR_ALBEDO) == (1, 2, 4, 8)
    assert A.ATTR_FLOATS == {1: 4, 2: 2, 4: 4, 8: 4}


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_attribute_calls():
    g.build()
    assert not set(A.ATTRIBUTE_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_attributes


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.ATTRIBUTE_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_attributes


def test_header_compiles_as_c():
    src = ('#include "svr_attributes.h"\n'
           'int main(void) { void* p = 0; int (*f)(SvrContext*, int, void*, size_t) = svr_read_attribute;\n'
           '  int (*e)(SvrContext*, uint32_t) = svr_enable_attributes;\n'
           '  return (p != 0) + (f == 0) + (e == 0) + (SVR_ATTR_ALL != (SVR_ATTR_BARY | SVR_ATTR_UV | SVR_ATTR_NORMAL | SVR_ATTR_ALBEDO)); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    buf = (C.c_float * 4)()
    p = C.c_void_p()
    assert L.svr_enable_attributes(None, A.ATTR_ALL) == -1
    assert L.svr_bind_attribute_target(None, A.ATTR_UV, None) == -1
    assert L.svr_get_attribute_target(None, A.ATTR_UV, C.byref(p)) == -1
    assert L.svr_read_attribute(None, A.ATTR_UV, buf, 16) == -1
    assert b"null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    for call in (lambda: r.enable_attributes(), lambda: r.bind_attribute_target(A.ATTR_BARY, 0),
                 lambda: r.get_attribute_target(A.ATTR_BARY), lambda: r.read_attribute(A.ATTR_BARY)):
        with pytest.raises(pkg.SvrError, match="no attribute targets") as e:
            call()
        assert e.value.code == -5
