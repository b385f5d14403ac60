"""The caller's side of the ambient pass (include/svr_ambient.h): pixels_per_unit of glmath.py against host/svr_math.h bit
for bit, and what the number means."""
import os
import subprocess

import numpy as np

import __graft_entry__ as g
import native_ref as N

pkg = g.load_package()
GL = pkg.glmath
f32 = np.float32
HOST_DIR = os.path.join(g.PKG_DIR, "host")

PROBE_SRC = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "svr_math.h"
int main(int argc, char** argv) {
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < n; k++) {
    svrm::mat4 p;
    float height;
    if (std::fread(p.data(), 4, 16, f) != 16 || std::fread(&height, 4, 1, f) != 1) return 2;
    const float v = svrm::pixels_per_unit(p, height);
    uint32_t u;
    std::memcpy(&u, &v, 4);
    std::printf("%08x\n", u);
  }
  return 0;
}
'''


def cases():
    rng = np.random.default_rng(11)
    out = []
    for k in range(32):
        w, h = [(1700, 900), (130, 67), (3840, 2160), (64, 64)][k % 4]
        proj = GL.scene_data(GL.identity(), w, h)[1].copy()
        if k >= 8:
            proj[1][1] = f32(rng.uniform(-3, 3))
        out.append((proj, f32(h)))
    return out


def test_glmath_agrees_with_svr_math_bit_for_bit(tmp_path):
    src, data = tmp_path / "probe.cpp", tmp_path / "cases.bin"
    src.write_text(PROBE_SRC)
    exe = N.build(str(src), include=(HOST_DIR,), extra=("-Wall", "-Werror"))
    cs = cases()
    with open(data, "wb") as f:
        f.write(np.uint32(len(cs)).tobytes())
        for proj, h in cs:
            f.write(np.asarray(proj, f32).tobytes() + np.float32(h).tobytes())
    got = subprocess.run([str(exe), str(data)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    want = [f"{int(np.asarray(GL.pixels_per_unit(proj, h), f32).reshape(1).view(np.uint32)[0]):08x}" for proj, h in cs]
    assert got == want


def test_one_unit_at_w_1_spans_that_many_pixels():
    """two points one world unit apart vertically, at clip w = 1 in front of the camera, land pixels_per_unit pixels apart"""
    w, h = 1700, 900
    proj = GL.scene_data(GL.identity(), w, h)[1]
    ppu = GL.pixels_per_unit(proj, h)
    assert isinstance(ppu, np.floating) and ppu.dtype == f32 and ppu > 0
    a, b = GL.matvec(proj, (0.0, -0.5, -1.0, 1.0)), GL.matvec(proj, (0.0, 0.5, -1.0, 1.0))
    assert a[3] == 1.0 and b[3] == 1.0
    ya, yb = (a[1] / a[3]) * h / 2 + h / 2, (b[1] / b[3]) * h / 2 + h / 2
    assert abs(abs(float(ya - yb)) - float(ppu)) < 1e-3 * float(ppu)
