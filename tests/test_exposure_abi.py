"""Auto-exposure at the C boundary, without a GPU: include/svr_exposure.h against the binding and the product library's
exports, the struct layouts, the oracle's refusal, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as g

pkg = g.load_package()
A = pkg.abi
HEADER = os.path.join(g.ROOT, "include", "svr_exposure.h")
INCLUDE = os.path.join(g.ROOT, "include")
METER_FIELDS = ["key", "low_fraction", "high_fraction", "min_exposure", "max_exposure", "adapt"]
STATE_FIELDS = ["exposure", "target", "mean_log2", "counted", "black", "meters"]


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_match_binding():
    assert declared_symbols() == sorted(A.EXPOSURE_SYMBOLS) == [
        "svr_debug_read_exposure_histogram", "svr_get_exposure_state", "svr_meter_exposure", "svr_read_exposure", "svr_reset_exposure",
        "svr_set_post_auto_exposure"]
    for other in (A.SYMBOLS, A.ID_SYMBOLS, A.DRAW_LIST_SYMBOLS, A.VIEWS_SYMBOLS, A.DEPTH_SYMBOLS, A.OCCLUSION_SYMBOLS, A.ATTRIBUTE_SYMBOLS,
                  A.LIGHTING_SYMBOLS, A.LOAD_SYMBOLS, A.POST_SYMBOLS, A.TEMPORAL_SYMBOLS, A.AMBIENT_SYMBOLS):
        assert not set(A.EXPOSURE_SYMBOLS) & set(other)


def test_the_post_pass_keeps_its_interface():
    assert A.POST_SYMBOLS == ["svr_post_pass"] and C.sizeof(A.SvrPostPass) == 20


def test_header_constants_match_binding():
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(SVR_EXPOSURE_[A-Z_]+)\s+(\d+)", open(HEADER).read())}
    assert defines == {"SVR_EXPOSURE_BINS": A.EXPOSURE_BINS} and A.EXPOSURE_BINS == 256


LAYOUT_SRC = r'''
#include <stddef.h>
#include <stdio.h>
#include "svr_exposure.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("SvrExposureMeter %zu\n", sizeof(SvrExposureMeter));
  F(SvrExposureMeter, key); F(SvrExposureMeter, low_fraction); F(SvrExposureMeter, high_fraction); F(SvrExposureMeter, min_exposure);
  F(SvrExposureMeter, max_exposure); F(SvrExposureMeter, adapt);
  printf("SvrExposureState %zu\n", sizeof(SvrExposureState));
  F(SvrExposureState, exposure); F(SvrExposureState, target); F(SvrExposureState, mean_log2); F(SvrExposureState, counted);
  F(SvrExposureState, black); F(SvrExposureState, meters);
  return 0;
}
'''


def test_struct_layouts_match_binding(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_SRC)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for name, cls, fields in (("SvrExposureMeter", A.SvrExposureMeter, METER_FIELDS), ("SvrExposureState", A.SvrExposureState, STATE_FIELDS)):
        assert [f for f, _ in cls._fields_] == fields
        want[name] = C.sizeof(cls)
        for field in fields:
            want[f"{name}.{field}"] = getattr(cls, field).offset
    assert got == want
    assert got["SvrExposureMeter"] == 24 and got["SvrExposureState"] == 24
    assert [got[f"SvrExposureMeter.{f}"] for f in METER_FIELDS] == [0, 4, 8, 12, 16, 20]
    assert [got[f"SvrExposureState.{f}"] for f in STATE_FIELDS] == [0, 4, 8, 12, 16, 20]


def test_header_compiles_as_c():
    src = ('#include "svr_exposure.h"\n'
           'int main(void) { int (*m)(SvrContext*, const SvrExposureMeter*) = svr_meter_exposure;\n'
           '  int (*r)(SvrContext*) = svr_reset_exposure;\n'
           '  int (*a)(SvrContext*, int) = svr_set_post_auto_exposure;\n'
           '  int (*s)(SvrContext*, SvrExposureState*) = svr_read_exposure;\n'
           '  int (*h)(SvrContext*, uint32_t*, size_t) = svr_debug_read_exposure_histogram;\n'
           '  int (*d)(SvrContext*, const void**) = svr_get_exposure_state;\n'
           '  SvrExposureMeter p; SvrExposureState t; p.key = 0.18f; p.adapt = 1.0f; t.meters = 0u; t.exposure = p.key;\n'
           '  return (m == 0) + (r == 0) + (a == 0) + (s == 0) + (h == 0) + (d == 0) + (t.meters != 0u) + (SVR_EXPOSURE_BINS != 256); }\n')
    p = subprocess.run(["cc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-"],
                       input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_product_library_exports_auto_exposure():
    g.build()
    assert not set(A.EXPOSURE_SYMBOLS) - _exports(pkg.PRODUCT_LIBRARY)
    assert pkg.load_product_library().has_exposure


def test_oracle_exports_none_of_it(oracle):
    assert not set(A.EXPOSURE_SYMBOLS) & _exports(oracle.path)
    assert not oracle.has_exposure


def test_null_arguments_are_refused_without_a_device():
    L = pkg.load_product_library().lib
    m = A.SvrExposureMeter(0.18, 0.0, 1.0, 0.001, 1000.0, 1.0)
    assert L.svr_meter_exposure(None, C.byref(m)) == -1
    assert b"null" in L.svr_last_error()
    assert L.svr_meter_exposure(None, None) == -1
    st = A.SvrExposureState(exposure=7.0)
    buf = (C.c_uint32 * 256)()
    target = C.c_void_p(7)
    assert L.svr_reset_exposure(None) == -1
    assert L.svr_set_post_auto_exposure(None, 1) == -1
    assert L.svr_read_exposure(None, C.byref(st)) == -1 and st.exposure == 7.0
    assert L.svr_debug_read_exposure_histogram(None, buf, 1024) == -1
    assert L.svr_get_exposure_state(None, C.byref(target)) == -1 and target.value == 7
    assert b"null" in L.svr_last_error()


@pytest.mark.parametrize("call", ["meter_exposure", "reset_exposure", "set_post_auto_exposure", "read_exposure", "read_exposure_histogram",
                                  "exposure_state_ptr"])
def test_oracle_is_refused_cleanly(oracle, call):
    r = A.Renderer.__new__(A.Renderer)
    r.lib = oracle
    with pytest.raises(pkg.SvrError, match=r"has no auto-exposure \(include/svr_exposure.h\)") as e:
        getattr(r, call)()
    assert e.value.code == -5
