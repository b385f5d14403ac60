"""The depth loadOp at the C boundary, without a GPU: include/svr_load.h against the binding and the product library's
exports, the enum's values, a library without the calls, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_load.h")
INCLUDE = os.path.join(g.ROOT, "include")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.LOAD_SYMBOLS) == ["svr_get_depth_load_op", "svr_set_depth_load_op"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS):
        assert not set(A.LOAD_SYMBOLS) & set(other)


def test_header_compiles_as_c_and_the_enum_is_0_and_1(tmp_path):
    src, exe = tmp_path / "load.c", tmp_path / "load"
    src.write_text('#include <stdio.h>\n#include "svr_load.h"\n'
                   'int main(void) { int (*s)(SvrContext*, int) = svr_set_depth_load_op; int (*q)(SvrContext*, int*) = svr_get_depth_load_op;\n'
                   '  enum SvrDepthLoadOp op = SVR_DEPTH_LOAD; (void)s; (void)q;\n'
                   '  printf("%d %d %d\\n", (int)SVR_DEPTH_CLEAR, (int)SVR_DEPTH_LOAD, (int)op); return 0; }\n')
    # -c: the two calls are the HIP library's, nothing to link against here
    p = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "load.o"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    vals = tmp_path / "vals.c"
    vals.write_text('#include <stdio.h>\n#include "svr_load.h"\nint main(void) { printf("%d %d\\n", (int)SVR_DEPTH_CLEAR, (int)SVR_DEPTH_LOAD); return 0; }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(vals)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert [int(v) for v in out] == [0, 1] == [A.DEPTH_CLEAR, A.DEPTH_LOAD]


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_the_calls():
    g.build()
    assert not set(A.LOAD_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_depth_load


def test_a_library_without_them_loads(oracle):
    assert not set(A.LOAD_SYMBOLS) & _exports(oracle.path)
    assert oracle.has_depth_load is False
    r = oracle.create(8, 8)  # the rest of the binding works as before
    for call in (lambda: r.set_depth_load_op(A.DEPTH_LOAD), lambda: r.get_depth_load_op()):
        with pytest.raises(pkg.SvrError, match="no depth loadOp") as e:
            call()
        assert e.value.code == -5
    r.close()


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    op = C.c_int(7)
    assert L.svr_set_depth_load_op(None, A.DEPTH_LOAD) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_get_depth_load_op(None, C.byref(op)) == -1
    assert b"null" in L.svr_last_error()
    assert op.value == 7
