// frag_third_check.cpp — host check of two rewrites of the fragment stage's third cut, on the header's own code
// (tests/test_frag_third.py cuts it out of csrc/svr_device.h into frag_third_under_test.h):
//   1. lod_from_rho2<false> — the LOD chain without its upper range select — gives, under clamp_med3(., lo, hi) with
//      -50 <= lo <= hi <= 50, the bits lod_from_rho2<true> gives, for every rho2 >= 0, +inf and the NaNs included; and
//      binding_lod_range narrows a sampler's clamps into that interval without changing min(max(x, lo), hi) for any x
//      in [-50, 50], or reports the range as wide.
//   2. With edges 1 and 2 stored unbiased, f = g - u (coverage) and g (barycentrics) are the doubles the biased record's
//      chain produced as f and f + u, for integer edges of the sizes setup_triangle makes, ties included; and the bias
//      read off an edge's steps (binning) is the one the flags carry.
// Prints "lod <n> ranges <n> edges <n> ok"; any difference is printed and the exit status is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#define __host__
#define __device__
#define __forceinline__ inline
namespace under_test {
inline uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
using ::fmaf;
#include "frag_third_under_test.h"
}  // namespace under_test
using under_test::f2u;
using under_test::u2f;

// v_med3_f32 for operands that are not NaN: the median of the three
static float med3(float x, float lo, float hi) { return std::fmax(std::fmin(x, lo), std::fmin(std::fmax(x, lo), hi)); }

static int failures = 0;
static void fail(const char* what, double a, double b, double c, double d) {
  if (failures++ < 20) std::printf("FAIL %s: %.17g %.17g %.17g %.17g\n", what, a, b, c, d);
}

static const float CLAMPS[6][2] = {{-50.f, 50.f}, {0.f, 0.f}, {0.f, 10.f}, {3.5f, 3.5f}, {-50.f, -50.f}, {50.f, 50.f}};

static long check_lod_at(uint32_t bits) {
  const float rho2 = u2f(bits);
  const float with = under_test::lod_from_rho2<true>(rho2), without = under_test::lod_from_rho2<false>(rho2);
  for (const auto& c : CLAMPS) {
    const float a = med3(with, c[0], c[1]), b = med3(without, c[0], c[1]);
    if (f2u(a) != f2u(b)) fail("lod forms differ (rho2, lo, hi, with selects)", rho2, c[0], c[1], with);
  }
  return 6;
}

static long check_lod() {
  long n = 0;
  // every exponent field, the denormals' included, 2^16 evenly spaced mantissas each; the last field is +inf and the NaNs,
  // which the lower select — kept in both forms — sends to -50
  for (uint32_t e = 0; e < 256; e++)
    for (uint32_t k = 0; k < 65536u; k++) n += check_lod_at((e << 23) | (k << 7));
  const uint32_t hi = f2u(0x1p+100f), lo = f2u(0x1p-100f);
  const uint32_t points[] = {hi - 1, hi, hi + 1, lo - 1, lo, lo + 1, 0u, 1u, 0x007fffffu, 0x00800000u,
                             f2u(std::numeric_limits<float>::max()), f2u(std::numeric_limits<float>::infinity())};
  for (uint32_t p : points) n += check_lod_at(p);
  for (uint32_t d = 0; d < 4096u; d++) n += check_lod_at(hi - 2048u + d) + check_lod_at(lo - 2048u + d);  // every float around the two thresholds
  return n;
}

static long check_ranges() {
  const float S = under_test::LOD_SELECT;
  if (S != 50.0f) fail("LOD_SELECT", S, 0, 0, 0);
  const float ends[] = {-1000.f, -60.f, -50.5f, -50.f, -49.5f, -2.f, 0.f, 0.25f, 3.5f, 13.f, 49.5f, 50.f, 50.5f, 60.f, 1000.f};
  long n = 0;
  for (float lo : ends)
    for (float hi : ends) {
      if (!(lo <= hi)) continue;  // svr_create_sampler admits no other pair
      float nlo, nhi;
      const bool narrow = under_test::binding_lod_range(lo, hi, nlo, nhi);
      if (!(nlo <= nhi)) fail("range out of order", lo, hi, nlo, nhi);
      if (narrow != (nlo >= -S && nhi <= S)) fail("range verdict", lo, hi, nlo, nhi);
      if (narrow != !(lo > S || hi < -S)) fail("range withheld although it reaches [-50, 50]", lo, hi, nlo, nhi);
      if (!narrow && (nlo != lo || nhi != hi)) fail("wide range changed", lo, hi, nlo, nhi);
      for (int i = -400; i <= 400; i++) {  // every LOD a stage can clamp lies in [-50, 50]
        const float x = 0.125f * (float)i;
        const float a = std::fmin(std::fmax(x, lo), hi), b = std::fmin(std::fmax(x, nlo), nhi);
        if (f2u(a) != f2u(b)) fail("narrowed range changes a clamp (x, lo, hi, narrowed value)", x, lo, hi, b);
        if (narrow && f2u(med3(x, nlo, nhi)) != f2u(a)) fail("median differs from the chain", x, lo, hi, a);
        n++;
      }
    }
  return n;
}

// one edge at one pixel, the parent's chain against the change's.  Cu: the unbiased constant (an integer); u: 0 or 1
static void check_edge(double A, double B, long long Cu, int u, double px, double py, double dk) {
  const uint32_t flags = (u ? 1u : 0u) | (u ? 2u : 0u);
  const double u1 = under_test::edge_bias(flags, 1u), u2 = under_test::edge_bias(flags, 2u);
  if (u1 != (double)u || u2 != (double)u) fail("edge_bias(flags)", u1, u2, u, 0);
  const double Cb = (double)(Cu + (u ? -1 : 0)), C = (double)Cu;  // the record's constant: parent (biased), change (unbiased)
  // fragment stage, ordered scan: f (coverage) and g (barycentrics) at the pixel
  const double f_old = std::fma(A, px, std::fma(B, py, Cb)), g_old = f_old + u1;
  const double g_new = std::fma(A, px, std::fma(B, py, C)), f_new = g_new - u1;
  if (std::memcmp(&f_old, &f_new, 8) || std::memcmp(&g_old, &g_new, 8)) fail("f = g - u", f_old, f_new, g_old, g_new);
  if ((f_old >= 0.0) != (g_new >= u1)) fail("coverage predicate g >= u", f_old, g_new, u1, 0);
  // phase A: the span's first row, dk rows below
  const double s_old = std::fma(B, dk, f_old) + u1, s_new = std::fma(B, dk, g_new);
  if (std::memcmp(&s_old, &s_new, 8)) fail("span start", s_old, s_new, dk, 0);
}

static long check_edges() {
  std::mt19937_64 rng(20260903u);
  auto in = [&](long long lo, long long hi) { return (long long)(rng() % (unsigned long long)(hi - lo + 1)) + lo; };
  long n = 0;
  for (int it = 0; it < 400000; it++) {
    // edge steps as setup_triangle forms them: A = -256 dy, B = 256 dx, |A|, |B| <= 2^29
    const long long dy = in(-(1 << 21), 1 << 21), dx = in(-(1 << 21), 1 << 21);
    if (dx == 0 && dy == 0) continue;
    const double A = (double)(-dy * 256), B = (double)(dx * 256);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    if (under_test::edge_bias(A, B) != (top_left ? 0.0 : 1.0)) fail("edge_bias(A, B)", A, B, top_left, 0);
    const long long px = in(-32768, 32768), py = in(-32768, 32768), dk = in(0, 31);
    const long long at = -dy * 256 * px + dx * 256 * py;  // |.| < 2^46
    long long Cu = in(-(1ll << 52) + 1, (1ll << 52) - 1);
    for (int u = 0; u < 2; u++) {
      check_edge(A, B, Cu, u, (double)px, (double)py, (double)dk);
      check_edge(A, B, -at, u, (double)px, (double)py, (double)dk);      // a tie: g = 0 at the pixel
      check_edge(A, B, -at - 1, u, (double)px, (double)py, (double)dk);  // g = -1
      check_edge(A, B, -at + 1, u, (double)px, (double)py, (double)dk);  // g = 1: in whatever the bias
      n += 4;
    }
  }
  return n;
}

int main() {
  const long n_lod = check_lod(), n_ranges = check_ranges(), n_edges = check_edges();
  std::printf("lod %ld ranges %ld edges %ld %s\n", n_lod, n_ranges, n_edges, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
