// What the fragment stage's common case takes from setup (csrc/svr_device.h, the region tests/test_frag_setup.py cuts out):
//  1. tex_consts / packed_*: for every lw, lh in 0..14 and every level the forms that read the texture's packed constants
//     equal mip_offset, level_lw, level_lh and level_bytes.
//  2. frag_ranges_ok, soundness: seeded triangles are set up as setup_triangle does (snapped vertices, exact edge
//     functions, fp32 planes) and given to the predicate.  Whenever it says "common", a walk over every covered pixel
//     centre evaluates shade_pixel's fp32 chain with std::fmaf and checks that 1/w at the pixel and at both quad partners
//     passes the reciprocal's exponent window and that |u|, |v| < 2^23.  One violation fails the program.
//  3. frag_ranges_ok, usefulness: of the ordinary-camera family (triangles of random orientation in front of a pinhole
//     camera, w in [0.1, 1000], |uv| <= 64, and slivers 1/256 px wide cut from them) at least 99 % must stay common.
// Prints "... ok", or the first violation and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#define __host__
#define __device__
#include "frag_setup_under_test.h"

using namespace svr_layout;

// ---------------------------------------------------------------- 1. packed texture constants
static int check_consts(unsigned long long* n) {
  for (uint32_t lw = 0; lw <= 14; lw++)
    for (uint32_t lh = 0; lh <= 14; lh++) {
      const uint32_t levels = (lw > lh ? lw : lh) + 1u;
      const uint32_t k = tex_consts(lw, lh, levels), info = lw | (lh << 8) | (levels << 16) | (7u << 24);
      if ((k >> 24) != levels - 1u) return std::printf("lw %u lh %u: levels - 1 packed as %u\n", lw, lh, k >> 24), 1;
      for (uint32_t l = 0; l < levels; l++) {
        if (packed_mip_offset(k, l) != mip_offset(lw, lh, l) || packed_level_lw(info, l) != level_lw(lw, l) ||
            packed_level_lh(info, l) != level_lh(lh, l) || packed_level_bytes(k, l) != level_bytes(lw, lh, l))
          return std::printf("lw %u lh %u level %u: packed %u %u %u %u, closed forms %u %u %u %u\n", lw, lh, l, packed_mip_offset(k, l),
                             packed_level_lw(info, l), packed_level_lh(info, l), packed_level_bytes(k, l), mip_offset(lw, lh, l),
                             level_lw(lw, l), level_lh(lh, l), level_bytes(lw, lh, l)), 1;
        ++*n;
      }
    }
  return 0;
}

// ---------------------------------------------------------------- 2. the predicate against a walk
static uint64_t rng_state = 0x53505A41u;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static double uni(double a, double b) { return a + (b - a) * (double)(rnd64() >> 11) * 0x1p-53; }
static double logu(double a, double b) { return std::exp(uni(std::log(a), std::log(b))); }

struct Vtx {
  float xs, ys, w, u, v;  // screen position in pixels, clip w, texture coordinates
};
// the record's fields the fragment stage interpolates with, as setup_triangle forms them
struct Rec {
  int minx, miny, maxx, maxy;
  double A[3], B[3], C[3];
  bool t1, t2;
  float inv_area, q0, dq1, dq2, u0, du1, du2, v0, dv1, dv2;
  bool common;
};
constexpr int SCREEN_W = 1920, SCREEN_H = 1080;

static bool setup(const Vtx& p0, const Vtx& p1in, const Vtx& p2in, Rec& r) {
  Vtx p1 = p1in, p2 = p2in;
  auto snap = [](float f) { return (int)std::nearbyintf(f * 256.0f); };
  int X0 = snap(p0.xs), Y0 = snap(p0.ys), X1 = snap(p1.xs), Y1 = snap(p1.ys), X2 = snap(p2.xs), Y2 = snap(p2.ys);
  long long area2 = (long long)(X1 - X0) * (long long)(Y2 - Y0) - (long long)(X2 - X0) * (long long)(Y1 - Y0);
  if (area2 == 0) return false;
  if (area2 < 0) {
    int t;
    t = X1; X1 = X2; X2 = t;
    t = Y1; Y1 = Y2; Y2 = t;
    Vtx tv = p1; p1 = p2; p2 = tv;
    area2 = -area2;
  }
  auto min3 = [](int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); };
  auto max3 = [](int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); };
  r.minx = (min3(X0, X1, X2) + 127) >> 8, r.maxx = (max3(X0, X1, X2) - 128) >> 8;
  r.miny = (min3(Y0, Y1, Y2) + 127) >> 8, r.maxy = (max3(Y0, Y1, Y2) - 128) >> 8;
  if (r.minx < 0) r.minx = 0;
  if (r.miny < 0) r.miny = 0;
  if (r.maxx > SCREEN_W - 1) r.maxx = SCREEN_W - 1;
  if (r.maxy > SCREEN_H - 1) r.maxy = SCREEN_H - 1;
  if (r.minx > r.maxx || r.miny > r.maxy) return false;
  const int Xs[3] = {X0, X1, X2}, Ys[3] = {Y0, Y1, Y2};
  r.t1 = r.t2 = false;
  for (int i = 0; i < 3; i++) {
    const int a = (i + 1) % 3, b = (i + 2) % 3;
    const long long dx = (long long)Xs[b] - Xs[a], dy = (long long)Ys[b] - Ys[a];
    const long long Ae = -dy, Be = dx, Ce = -dx * Ys[a] + dy * Xs[a];
    const bool top_left = (dy < 0) || (dy == 0 && dx > 0);
    r.A[i] = (double)(Ae * 256);
    r.B[i] = (double)(Be * 256);
    r.C[i] = (double)(Ce + 128 * (Ae + Be) + (top_left ? 0 : -1));
    if (!top_left && i == 1) r.t1 = true;
    if (!top_left && i == 2) r.t2 = true;
  }
  r.inv_area = 1.0f / (float)(double)area2;
  const float rw0 = 1.0f / p0.w, rw1 = 1.0f / p1.w, rw2 = 1.0f / p2.w;  // the contract's IEEE 1/x
  r.q0 = rw0, r.dq1 = rw1 - rw0, r.dq2 = rw2 - rw0;
  const float u0 = p0.u * rw0, u1 = p1.u * rw1, u2 = p2.u * rw2, v0 = p0.v * rw0, v1 = p1.v * rw1, v2 = p2.v * rw2;
  r.u0 = u0, r.du1 = u1 - u0, r.du2 = u2 - u0;
  r.v0 = v0, r.dv1 = v1 - v0, r.dv2 = v2 - v0;
  const float uv[6] = {p0.u, p0.v, p1.u, p1.v, p2.u, p2.v};
  r.common = frag_ranges_ok(r.q0, r.dq1, r.dq2, r.A[1], r.B[1], r.A[2], r.B[2], r.inv_area, uv);
  return true;
}

static bool in_window(float x) {  // rcp_fast_ok
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return ((b >> 23) & 0xffu) - 32u <= 190u;
}
static float interp3(float a0, float da1, float da2, float b1, float b2, float r) { return std::fmaf(b2, da2, std::fmaf(b1, da1, a0)) * r; }

// every covered pixel of a triangle the predicate called common: 0 = all in range
static int walk(const Rec& t, const char* family, unsigned long long* n_pixels) {
  for (int py = t.miny; py <= t.maxy; py++)
    for (int px = t.minx; px <= t.maxx; px++) {
      const double dx = px, dy = py;
      const double e0 = std::fma(t.A[0], dx, std::fma(t.B[0], dy, t.C[0]));
      double e1 = std::fma(t.A[1], dx, std::fma(t.B[1], dy, t.C[1])), e2 = std::fma(t.A[2], dx, std::fma(t.B[2], dy, t.C[2]));
      if (e0 < 0.0 || e1 < 0.0 || e2 < 0.0) continue;
      ++*n_pixels;
      e1 += t.t1 ? 1.0 : 0.0;
      e2 += t.t2 ? 1.0 : 0.0;
      const float b1 = (float)e1 * t.inv_area, b2 = (float)e2 * t.inv_area;
      const float qq = std::fmaf(b2, t.dq2, std::fmaf(b1, t.dq1, t.q0));
      const double sxp = (px & 1) ? -1.0 : 1.0, syp = (py & 1) ? -1.0 : 1.0;
      const float hb1 = (float)std::fma(sxp, t.A[1], e1) * t.inv_area, hb2 = (float)std::fma(sxp, t.A[2], e2) * t.inv_area;
      const float vb1 = (float)std::fma(syp, t.B[1], e1) * t.inv_area, vb2 = (float)std::fma(syp, t.B[2], e2) * t.inv_area;
      const float hq = std::fmaf(hb2, t.dq2, std::fmaf(hb1, t.dq1, t.q0)), vq = std::fmaf(vb2, t.dq2, std::fmaf(vb1, t.dq1, t.q0));
      if (!in_window(qq) || !in_window(hq) || !in_window(vq))
        return std::printf("%s: pixel (%d,%d): 1/w %a, partners %a %a outside the reciprocal's window\n", family, px, py, qq, hq, vq), 1;
      const float r = 1.0f / qq;
      const float u = interp3(t.u0, t.du1, t.du2, b1, b2, r), v = interp3(t.v0, t.dv1, t.dv2, b1, b2, r);
      if (!(std::fabs(u) < 8388608.0f) || !(std::fabs(v) < 8388608.0f))
        return std::printf("%s: pixel (%d,%d): u %a v %a not below 2^23\n", family, px, py, u, v), 1;
    }
  return 0;
}

struct Tally {
  unsigned long long tris = 0, common = 0;
};
static unsigned long long g_pixels = 0;
static int submit(const Vtx& a, const Vtx& b, const Vtx& c, const char* family, Tally& t) {
  Rec r;
  if (!setup(a, b, c, r)) return 0;
  t.tris++;
  if (!r.common) return 0;
  t.common++;
  return walk(r, family, &g_pixels);
}

// A triangle of random orientation in front of a pinhole camera (focal length 1000 px): centre at depth zc, corners
// within rho * zc of it, every corner's depth kept inside [0.1, 1000]
static void camera_triangle(Vtx (&p)[3], double uvmax) {
  const double f = 1000.0, zc = logu(0.15, 700.0), rho = logu(0.002, 0.4);
  const double cx = uni(-1.0, 1.0) * zc, cy = uni(-0.6, 0.6) * zc;
  for (int i = 0; i < 3; i++) {
    double z = zc + uni(-1.0, 1.0) * rho * zc;
    z = z < 0.1 ? 0.1 : (z > 1000.0 ? 1000.0 : z);
    const double x = cx + uni(-1.0, 1.0) * rho * zc, y = cy + uni(-1.0, 1.0) * rho * zc;
    p[i].xs = (float)(960.0 + f * x / z);
    p[i].ys = (float)(540.0 + f * y / z);
    p[i].w = (float)z;
    p[i].u = (float)uni(-uvmax, uvmax);
    p[i].v = (float)uni(-uvmax, uvmax);
  }
}
// corner 2 moved to `width` pixels beside corner 1, across the edge 0-1; its w and uv follow unless `own_w`
static void make_sliver(Vtx (&p)[3], double width, bool own_w) {
  // at most 96 px long (the walk visits the bounding box), from corner 0 towards corner 1
  double ex = p[1].xs - p[0].xs, ey = p[1].ys - p[0].ys, len = std::sqrt(ex * ex + ey * ey);
  if (len < 4.0) ex = 37.0, ey = 5.0, len = std::sqrt(ex * ex + ey * ey);
  const double want = len > 96.0 ? 96.0 : len;
  const float w1 = p[1].w;
  p[1].xs = (float)(p[0].xs + ex / len * want);
  p[1].ys = (float)(p[0].ys + ey / len * want);
  p[1].w = (float)(p[0].w + (w1 - p[0].w) * want / len);
  const float keep_w = p[2].w;
  p[2] = p[1];
  p[2].xs = (float)(p[1].xs - ey / len * width);
  p[2].ys = (float)(p[1].ys + ex / len * width);
  p[2].w = own_w ? keep_w : p[1].w * (1.0f + (float)uni(-1.0, 1.0) * 0x1p-18f);  // as thin in depth as on the screen
}

int main() {
  unsigned long long n_consts = 0;
  if (check_consts(&n_consts)) return 1;

  Tally ordinary, sliver, grazing, scaled, bigtex, nonfinite;
  Vtx p[3];
  // ordinary cameras, and slivers cut from them (1/256 px wide; every fourth two wide so that pixel centres fall inside)
  for (int i = 0; i < 6000; i++) {
    camera_triangle(p, 64.0);
    if (submit(p[0], p[1], p[2], "ordinary", ordinary)) return 1;
  }
  for (int i = 0; i < 3000; i++) {
    camera_triangle(p, 64.0);
    make_sliver(p, (i & 3) ? 1.0 / 256.0 : 2.0 / 256.0, false);
    if (i & 1) {  // along a row of pixel centres: the sliver covers every centre between its ends
      p[0].ys = p[1].ys = std::floor(p[0].ys) + 0.5f;
      p[2].xs = p[1].xs;
      p[2].ys = p[1].ys + ((i & 3) == 1 ? 1.0f : 2.0f) / 256.0f;
      p[0].ys += 0.5f / 256.0f * ((i & 3) == 1 ? 0.0f : 2.0f);
    }
    if (submit(p[0], p[1], p[2], "ordinary sliver", ordinary)) return 1;
  }
  // adversarial slivers: the third corner keeps a depth of its own, so 1/w changes sign within a pixel of the triangle
  for (int i = 0; i < 6000; i++) {
    camera_triangle(p, 64.0);
    if (i & 1) p[2].w = (float)(p[1].w * (1.0 + uni(-1.0, 1.0) * logu(1e-7, 1e-1)));
    make_sliver(p, 1.0 / 256.0, true);
    if (submit(p[0], p[1], p[2], "sliver", sliver)) return 1;
  }
  // grazing planes: 1/w = g * (x - xh) + tilt * y, the far corners within 2 px of the horizon x = xh
  for (int i = 0; i < 6000; i++) {
    const double xh = uni(100.0, 1500.0), yc = uni(100.0, 900.0), g = logu(1e-4, 1.0), tilt = (i & 1) ? 0.0 : g * uni(-0.05, 0.05);
    const double d0 = logu(0.004, 2.0), d1 = logu(0.004, 2.0);
    const double xy[3][2] = {{xh + d0, yc + uni(-30.0, 30.0)}, {xh + d1, yc + uni(-30.0, 30.0)}, {xh + uni(3.0, 80.0), yc + uni(-30.0, 30.0)}};
    bool ok = true;
    for (int k = 0; k < 3; k++) {
      const double q = g * (xy[k][0] - xh) + tilt * (xy[k][1] - yc);
      ok = ok && q > 0.0;
      p[k].xs = (float)xy[k][0];
      p[k].ys = (float)xy[k][1];
      p[k].w = (float)(1.0 / q);
      p[k].u = (float)uni(-64.0, 64.0);
      p[k].v = (float)uni(-64.0, 64.0);
    }
    if (ok && submit(p[0], p[1], p[2], "grazing", grazing)) return 1;
  }
  // w scaled by powers of two: the window's ends
  const int scales[] = {40, -40, 70, -70, 88, -88, 93, -93, 96, -96, 100, -100};
  for (int s : scales)
    for (int i = 0; i < 400; i++) {
      camera_triangle(p, 64.0);
      if (i & 1) make_sliver(p, 1.0 / 256.0, false);
      for (int k = 0; k < 3; k++) p[k].w = std::ldexp(p[k].w, s);
      if (submit(p[0], p[1], p[2], "scaled w", scaled)) return 1;
    }
  // texture coordinates at the guard's limit
  const float big[] = {4194303.0f, 4194304.0f, 8388608.0f, 4194304.0f * (1.0f - 0x1p-10f), 4194304.0f * (1.0f - 0x1p-16f), 2097152.0f, 8388607.5f, 1.0e9f};
  for (float b : big)
    for (int i = 0; i < 300; i++) {
      camera_triangle(p, 64.0);
      const int k = (int)(rnd64() % 3u);
      ((i & 1) ? p[k].u : p[k].v) = (i & 2) ? -b : b;
      if (i & 4) p[(k + 1) % 3].u = b, p[(k + 2) % 3].u = b;
      if (submit(p[0], p[1], p[2], "large uv", bigtex)) return 1;
    }
  // infinite and NaN coordinates: never common
  const float bad[] = {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  for (float b : bad)
    for (int i = 0; i < 300; i++) {
      camera_triangle(p, 64.0);
      ((i & 1) ? p[i % 3].u : p[i % 3].v) = b;
      if (submit(p[0], p[1], p[2], "non-finite uv", nonfinite)) return 1;
    }
  if (nonfinite.common) return std::printf("non-finite uv: %llu triangles stayed common\n", nonfinite.common), 1;
  for (int i = 0; i < 300; i++) {  // ... and a non-finite or non-positive w
    camera_triangle(p, 64.0);
    const float ws[] = {0.0f, -1.0f, bad[0], bad[2], -0.0f};
    p[i % 3].w = ws[i % 5];
    Tally t;
    if (submit(p[0], p[1], p[2], "bad w", t)) return 1;
    if (t.common) return std::printf("bad w %a: the triangle stayed common\n", ws[i % 5]), 1;
  }

  const double keep = (double)ordinary.common / (double)ordinary.tris;
  std::printf("consts %llu ordinary %llu/%llu sliver %llu/%llu grazing %llu/%llu scaled %llu/%llu large-uv %llu/%llu pixels %llu keep %.4f\n", n_consts,
              ordinary.common, ordinary.tris, sliver.common, sliver.tris, grazing.common, grazing.tris, scaled.common, scaled.tris,
              bigtex.common, bigtex.tris, g_pixels, keep);
  // every adversarial family must exercise BOTH answers, or it tests nothing
  const Tally* both[] = {&sliver, &grazing, &scaled, &bigtex};
  for (const Tally* t : both)
    if (t->common == 0 || t->common == t->tris) return std::printf("a family has only one answer\n"), 1;
  if (keep < 0.99) return std::printf("the predicate keeps %.4f of the ordinary family: below 0.99\n", keep), 1;
  std::printf("ok\n");
  return 0;
}
