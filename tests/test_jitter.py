"""The caller's side of temporal antialiasing (include/svr_temporal.h): halton, jitter_projection and temporal_reproject of
glmath.py against host/svr_math.h bit for bit, the size and the sign of the jitter."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as g
import native_ref as N
import scenarios as SC

pkg = g.load_package()
A, S, GL = pkg.abi, pkg.scenes, pkg.glmath
f32 = np.float32
HOST_DIR = os.path.join(g.PKG_DIR, "host")

PROBE_SRC = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "svr_math.h"
static void put(const float* v, int n) {
  for (int i = 0; i < n; i++) { uint32_t u; std::memcpy(&u, &v[i], 4); std::printf("%08x ", u); }
  std::printf("\n");
}
int main(int argc, char** argv) {
  for (unsigned base = 2; base <= 5; base++)
    for (unsigned i = 0; i < 40; i++) { float h = svrm::halton(i, base); put(&h, 1); }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < n; k++) {
    svrm::mat4 a, b;
    float j[4];
    if (std::fread(a.data(), 4, 16, f) != 16 || std::fread(b.data(), 4, 16, f) != 16 || std::fread(j, 4, 4, f) != 4) return 2;
    svrm::mat4 p = svrm::jitter_projection(a, j[0], j[1], j[2], j[3]);
    put(p.data(), 16);
    svrm::mat4 r = svrm::temporal_reproject(a, b);
    put(r.data(), 16);
  }
  return 0;
}
'''


def bits(v):
    return " ".join(f"{int(x):08x}" for x in np.asarray(v, f32).reshape(-1).view(np.uint32)) + " "


def cases():
    rng = np.random.default_rng(5)
    out = []
    for k in range(24):
        w, h = [(1700, 900), (130, 67), (3840, 2160), (64, 64)][k % 4]
        pos = tuple(rng.uniform(-5, 5, 3))
        pitch, yaw = float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-3, 3))
        a = GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[2]
        b = GL.scene_data(GL.camera_view(tuple(np.add(pos, rng.normal(0, 0.2, 3))), pitch + float(rng.normal(0, 0.02)), yaw + float(rng.normal(0, 0.05))), w, h)[2]
        if k % 6 == 5:
            b = a  # a static camera
        j = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), w, h], f32)
        out.append((a, b, j))
    return out


def test_glmath_agrees_with_svr_math_bit_for_bit(tmp_path):
    src, data = tmp_path / "probe.cpp", tmp_path / "cases.bin"
    src.write_text(PROBE_SRC)
    exe = N.build(str(src), include=(HOST_DIR,), extra=("-Wall", "-Werror"))
    cs = cases()
    with open(data, "wb") as f:
        f.write(np.uint32(len(cs)).tobytes())
        for a, b, j in cs:
            f.write(np.asarray(a, f32).tobytes() + np.asarray(b, f32).tobytes() + j.tobytes())
    got = subprocess.run([str(exe), str(data)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    want = [bits(GL.halton(i, base)) for base in range(2, 6) for i in range(40)]
    for a, b, j in cs:
        want.append(bits(GL.jitter_projection(a, j[0], j[1], j[2], j[3])))
        want.append(bits(GL.temporal_reproject(a, b)))
    assert len(got) == len(want)
    for k, (x, y) in enumerate(zip(got, want)):
        assert x == y, f"line {k}"


def test_halton_values():
    assert [float(GL.halton(i, 2)) for i in range(1, 8)] == [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875]
    assert [GL.halton(i, 3) for i in range(1, 5)] == [f32(1 / 3), f32(2 / 3), f32(1 / 9), f32(4 / 9)]
    assert GL.halton(0, 2) == 0
    pts = np.array([[GL.halton(i, 2), GL.halton(i, 3)] for i in range(1, 17)], np.float64) - 0.5
    assert np.all(np.abs(pts) < 0.5) and len({tuple(p) for p in pts}) == 16
    assert np.abs(pts.mean(0)).max() < 0.05, "the 16 jitters of a period are centred on the pixel centre"


def test_static_camera_reprojects_to_the_identity():
    vp = GL.scene_data(GL.camera_view((1.0, 2.0, -3.0), 0.2, 0.7), 1700, 900)[2]
    m = np.asarray(GL.temporal_reproject(vp, vp), np.float64)
    assert np.abs(m - np.eye(4)).max() < 1e-6


@pytest.mark.parametrize("size", [(1700, 900), (130, 67)])
def test_a_jittered_point_moves_by_the_jitter(size):
    """view-space points through proj and through jitter_projection(proj), both read as exact (float64) matrices: the pixel
    position moves by (jx, jy) up to the rounding of the jittered matrix's entries.  u = 2^-24.  ax = (2 jx) / w is one
    rounding, ax * p[c][3] another, the sum a third, each relative to at most |p[c][0]| + |ax p[c][3]|, so the clip x of
    a point v is off by at most 3 u sum_c |v_c| (|p[c][0]| + |ax p[c][3]|), and the pixel by W / 2 of that over |w|."""
    w, h = size
    proj = GL.scene_data(GL.identity(), w, h)[1]
    rng = np.random.default_rng(9)
    v = np.concatenate([rng.uniform(-3, 3, (200, 2)), -rng.uniform(0.2, 50, (200, 1)), np.ones((200, 1))], axis=1)
    P = np.asarray(proj, np.float64).T  # [row][col]

    def pixels(M):
        clip = v @ M.T
        return np.stack([clip[:, 0] / clip[:, 3] * w / 2 + w / 2, clip[:, 1] / clip[:, 3] * h / 2 + h / 2], 1), clip[:, 3]

    base, cw = pixels(P)
    assert (cw > 0).all()
    u = 2.0 ** -24
    for jx, jy in ((0.25, -0.4), (-0.5, 0.5), (0.4375, 0.0)):
        J = np.asarray(GL.jitter_projection(proj, jx, jy, w, h), np.float64).T
        moved, _ = pixels(J)
        for axis, (jit, n) in enumerate(((jx, w), (jy, h))):
            a = 2.0 * jit / n
            s = np.abs(v) @ (np.abs(P[axis]) + np.abs(a * P[3]))
            bound = 3 * u * s * (n / 2) / cw
            err = np.abs(moved[:, axis] - base[:, axis] - jit)
            assert (err <= bound).all(), (jx, jy, axis, err.max(), bound.min())
            assert bound.max() < 1e-3


def test_the_sign_of_the_jitter_on_the_oracle(oracle):
    """a quad whose right edge runs through pixel column 10 at x = 10.6: the column's centres (10.5) are covered.  A
    jitter of +0.3 pixels moves the edge to 10.9 and keeps them; -0.3 moves it to 10.3 and loses them."""
    n, col = 32, 10
    edge = (col + 0.6) / (n / 2) - 1.0
    covered = {}
    for jx in (0.0, 0.3, -0.3):
        rig = SC.Rig(oracle, n, n, background=(0, 0, 0, 1))
        mesh = rig.r.upload_mesh(SC.QUAD_IDX, SC.clip_quad(-1, -1, edge, 1, 0.5))
        pj = GL.jitter_projection(GL.identity(), jx, 0.0, n, n)
        rig.draw(A.scene_struct(GL.identity(), pj, pj, [0.1] * 4, (0, 1, 0.5, 1), (1, 1, 1, 1)), [SC.render_object(mesh, rig.material(), 0, 6)])
        color = rig.finish()["color"]
        covered[jx] = (color[..., 0] != 0)
    for jx, cols in ((0.0, col + 1), (0.3, col + 1), (-0.3, col)):
        want = np.zeros((n, n), bool)
        want[:, :cols] = True
        assert np.array_equal(covered[jx], want), jx
