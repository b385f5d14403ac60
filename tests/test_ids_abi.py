"""The ID target at the C boundary, without a GPU: include/svr_ids.h against the binding and the product library's
exports, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_ids.h")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.ID_SYMBOLS)
    assert not set(A.ID_SYMBOLS) & set(A.SYMBOLS)  # the oracle's ABI (svr.h) is unchanged


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_id_calls():
    g.build()
    assert not set(A.ID_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_ids


def test_oracle_exports_none_of_them(oracle):
    assert not set(A.ID_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_ids


def test_header_compiles_as_c():
    src = ('#include "svr_ids.h"\n'
           'int main(void) { uint32_t id[2] = {0, 0}; int (*f)(SvrContext*, uint32_t, uint32_t, uint32_t*) = svr_pick;\n'
           '  return (int)id[0] + (f == 0); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(g.ROOT, "include"), "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def test_record_words_match_the_device_structs():
    text = open(os.path.join(g.PKG_DIR, "csrc", "svr_device.h")).read()
    assert 'offsetof(TriRec, object) == 240' in text and "uint32_t object, primitive;" in text


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    out = (C.c_uint32 * 2)()
    p = C.c_void_p()
    assert L.svr_enable_ids(None, 1) == -1
    assert L.svr_bind_id_target(None, None) == -1
    assert L.svr_get_id_target(None, C.byref(p)) == -1
    assert L.svr_read_ids(None, out, 8) == -1
    assert L.svr_pick(None, 0, 0, out) == -1
    assert b"null" in L.svr_last_error()


def test_oracle_is_refused_cleanly(oracle):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    for call in (lambda: r.enable_ids(), lambda: r.bind_id_target(0), lambda: r.get_id_target(), lambda: r.read_ids(),
                 lambda: r.pick(0, 0)):
        with pytest.raises(pkg.SvrError, match="no ID target"):
            call()
