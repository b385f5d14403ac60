// The identities the common-case fragment stage (csrc/k_tile.hip shade_pixel<.., COMMON>) is written with, checked in the
// host's IEEE arithmetic (built with -ffp-contract=off; every fma below is a std::fma call):
//  1. extents by exponent: ldexpf(f, k) has the bits of f * (float)(1 << k), for f in [0, 1) (the wrapped coordinate of
//     level_taps_exp) and for every finite d (the derivatives scaled by the extent), results that are denormal or
//     overflow included; k covers every level exponent an image of up to 16384 texels a side can have, and a few more.
//  2. clamps as medians: v_med3_f32 (stated below as the ISA documents it) equals fminf(fmaxf(x, lo), hi) as the hardware
//     evaluates it, for lo <= hi and every x that is not a NaN; and for lo > hi after binding_min_lod (csrc/svr_device.h,
//     the header's own code) has normalised the pair, where today's chain gives hi.
//  3. the derivative selects: a - b is -(b - a) bit for bit but for a zero's sign, and rho2 built from either is the same bits.
//  4. the partners' signs: e + A with A's sign bit flipped by the parity is fma(+-1, A, e), for integers up to 2^53.
// Prints "... ok", or the first violation and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define __host__
#define __device__
#include "frag_setup_under_test.h"

using svr_layout::binding_min_lod;

static uint64_t rng_state = 0x46524147u;
static uint64_t rnd64() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t d2u(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
static double u2d(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
static bool finite_bits(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------- 1. ldexpf against the product
static bool same_scaling(float f, int k, const char* what) {
  const float a = std::ldexp(f, k), b = f * (float)(1u << k);
  if (f2u(a) == f2u(b)) return true;
  std::printf("%s: f %a (%08x) k %d: ldexpf %a, product %a\n", what, f, f2u(f), k, a, b);
  return false;
}
static int check_scaling(unsigned long long* n) {
  // [0, 1): both ends, the denormals' ends and the values beside every one of them, with every k
  const uint32_t ends[] = {0u, 1u, 2u, 0x007ffffeu, 0x007fffffu, 0x00800000u, 0x00800001u, 0x00ffffffu, 0x01000000u,
                           0x3effffffu, 0x3f000000u, 0x3f000001u, 0x3f7ffffeu, 0x3f7fffffu, 0x33800000u, 0x34000000u};
  for (uint32_t e : ends)
    for (int k = 0; k <= 16; k++, ++*n)
      if (!same_scaling(u2f(e), k, "frac")) return 1;
  for (uint32_t i = 0; i < 12000000u; i++, ++*n)  // every bit pattern below 1.0f is equally likely: denormals, tiny and ordinary values
    if (!same_scaling(u2f((uint32_t)(rnd64() % 0x3f800000ull)), (int)(i % 17u), "frac")) return 1;
  // finite d of either sign: products that stay denormal, and products that overflow
  const uint32_t dends[] = {0u, 1u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f000000u, 0x7effffffu, 0x78800000u, 0x787fffffu, 0x3f800000u};
  for (uint32_t e : dends)
    for (uint32_t s = 0; s < 2; s++)
      for (int k = 0; k <= 16; k++, ++*n)
        if (!same_scaling(u2f(e | (s << 31)), k, "derivative")) return 1;
  for (uint32_t i = 0; i < 12000000u; ++*n) {
    const uint32_t b = (uint32_t)rnd64();
    if (!finite_bits(b)) continue;
    if (!same_scaling(u2f(b), (int)(i % 17u), "derivative")) return 1;
    i++;
  }
  return 0;
}

// ---------------------------------------------------------------- 2. the median against the chain
// v_max_f32 / v_min_f32 / v_med3_f32 with IEEE mode on, for operands that are not NaN: -0 orders below +0
static bool below(float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }
static float hw_max(float a, float b) { return below(a, b) ? b : a; }
static float hw_min(float a, float b) { return below(b, a) ? b : a; }
static float hw_med3(float a, float b, float c) {  // the ISA's statement: the largest is dropped, the larger of the rest stays
  const float m = hw_max(hw_max(a, b), c);
  if (f2u(m) == f2u(a)) return hw_max(b, c);
  if (f2u(m) == f2u(b)) return hw_max(a, c);
  return hw_max(a, b);
}
static int check_median(unsigned long long* n) {
  const float inf = INFINITY;
  const float xs[] = {0.0f, -0.0f, inf, -inf, 50.0f, -50.0f, 1.5f, 3.25f, 2.0f, -2.0f, 0.5f, 1000.0f, 16.0f, 1.4999999f, 1.5000001f,
                      3.2499998f, 3.2500002f, -63.5f, 64.0f, 0x1p-149f, -0x1p-149f, 1.0f, 3.0f};
  const float bounds[] = {0.0f, -0.0f, 1000.0f, 1.5f, 3.25f, -2.0f, 0.5f, 2.0f, 3.0f, 1.0f, 16.0f, -50.0f, 50.0f, inf, -inf, 7.0f};
  auto one = [&](float x, float lo, float hi) {
    const float chain = hw_min(hw_max(x, lo), hi);  // today's spelling, with the pair as the sampler gave it
    const float nlo = binding_min_lod(lo, hi);      // the pair as the binding carries it
    const float med = hw_med3(x, nlo, hi), chain2 = hw_min(hw_max(x, nlo), hi);
    ++*n;
    // a zero's sign is the one thing allowed to differ where lo and hi are zeros of either sign (the stage reads the clamp
    // through floor and a difference, which give the same bits for either zero)
    const bool ok = (f2u(med) == f2u(chain) || (med == 0.0f && chain == 0.0f)) && (f2u(chain2) == f2u(chain) || (chain2 == 0.0f && chain == 0.0f));
    if (!ok) std::printf("median: x %a lo %a hi %a: chain %a, median %a, chain on the normalised pair %a\n", x, lo, hi, chain, med, chain2);
    if (lo > hi && f2u(chain) != f2u(hi)) return std::printf("chain with lo %a > hi %a is not hi for x %a\n", lo, hi, x), false;
    return ok;
  };
  for (float lo : bounds)
    for (float hi : bounds)
      for (float x : xs)
        if (!one(x, lo, hi)) return 1;
  for (uint32_t i = 0; i < 4000000u; i++) {
    uint32_t b[3];
    for (uint32_t& v : b) do v = (uint32_t)rnd64(); while ((v & 0x7fffffffu) > 0x7f800000u);  // (no NaN; infinities stay)
    if (i & 1u) b[1] = (b[1] & 0x80000000u) | ((b[1] & 0x7fffffffu) % 0x42000000u), b[2] = (b[2] & 0x80000000u) | ((b[2] & 0x7fffffffu) % 0x42000000u);
    if (!one(u2f(b[0]), u2f(b[1]), u2f(b[2]))) return 1;
    if (!one(u2f(b[1]), u2f(b[1]), u2f(b[2])) || !one(u2f(b[2]), u2f(b[1]), u2f(b[2]))) return 1;  // x at a bound
  }
  // the level clamp: lc = clamp(lambda, 0, q), q = 0..16
  for (int q = 0; q <= 16; q++)
    for (float x : xs)
      if (!one(x, 0.0f, (float)q)) return 1;
  return 0;
}

// ---------------------------------------------------------------- 3. the derivatives without their selects
static float rho2_of(float dudx, float dvdx, float dudy, float dvdy, int lw, int lh) {
  const float mx = std::ldexp(dudx, lw), my = std::ldexp(dvdx, lh), nx = std::ldexp(dudy, lw), ny = std::ldexp(dvdy, lh);
  return std::fmax(std::fma(mx, mx, my * my), std::fma(nx, nx, ny * ny));
}
static int check_derivatives(unsigned long long* n) {
  const uint32_t ends[] = {0u, 0x80000000u, 1u, 0x80000001u, 0x00800000u, 0x3f800000u, 0xbf800000u, 0x3f800001u, 0x4b000000u, 0xcb000000u,
                           0x7f7fffffu, 0xff7fffffu, 0x3f000000u, 0x34000000u};
  auto one = [&](float u, float p, float v, float pv, int lw, int lh) {
    const float a = u - p, b = p - u;  // the odd column's and the even column's derivative
    ++*n;
    if (f2u(a) != (f2u(b) ^ 0x80000000u) && !(a == 0.0f && b == 0.0f)) return std::printf("u %a p %a: u - p %a, p - u %a\n", u, p, a, b), false;
    const float c = v - pv, d = pv - v;
    // the four sign combinations of (x parity, y parity) against the unselected form
    const float want = rho2_of(b, d, b, d, lw, lh);
    const float got[3] = {rho2_of(a, c, b, d, lw, lh), rho2_of(b, d, a, c, lw, lh), rho2_of(a, c, a, c, lw, lh)};
    for (float g : got)
      if (f2u(g) != f2u(want) && !(std::isnan(g) && std::isnan(want))) return std::printf("rho2: u %a p %a v %a pv %a: %a against %a\n", u, p, v, pv, g, want), false;
    return true;
  };
  for (uint32_t a : ends)
    for (uint32_t b : ends)
      if (!one(u2f(a), u2f(b), u2f(b), u2f(a), 10, 3)) return 1;
  for (uint32_t i = 0; i < 3000000u; i++) {
    uint32_t b[4];
    for (uint32_t& v : b) do v = (uint32_t)rnd64(); while (!finite_bits(v));
    if (i & 1u)  // neighbours, as a pixel and its quad partner are: the difference is small and often exact
      b[1] = b[0] + (uint32_t)(rnd64() % 64u) - 32u, b[3] = b[2] + (uint32_t)(rnd64() % 64u) - 32u;
    if (!finite_bits(b[1]) || !finite_bits(b[3])) continue;
    if (!one(u2f(b[0]), u2f(b[1]), u2f(b[2]), u2f(b[3]), (int)(i % 15u), (int)((i / 15u) % 15u))) return 1;
  }
  return 0;
}

// ---------------------------------------------------------------- 4. the partners' edge values
static double flip(double a, uint32_t parity) { return u2d(d2u(a) ^ ((uint64_t)(parity << 31) << 32)); }  // as the stage does: the high word's top bit
static int check_partners(unsigned long long* n) {
  const double ends[] = {0.0, 1.0, 255.0, 256.0, 0x1p24, 0x1p32 - 256.0, 0x1p52, 0x1p53 - 1.0, 0x1p53};
  auto one = [&](double e, double A) {
    for (uint32_t parity = 0; parity < 2; parity++, ++*n) {
      const double want = std::fma(parity ? -1.0 : 1.0, A, e), got = e + flip(A, parity);
      if (d2u(want) != d2u(got)) return std::printf("partners: e %a A %a parity %u: fma %a, sum %a\n", e, A, parity, want, got), false;
    }
    return true;
  };
  for (double e : ends)
    for (double A : ends)
      for (int s = 0; s < 4; s++)
        if (!one((s & 1) ? -e : e, (s & 2) ? -A : A)) return 1;
  for (uint32_t i = 0; i < 3000000u; i++) {
    // edge values are integers below 2^53 in magnitude, steps are integers times 256 below 2^32
    const int sh = (int)(rnd64() % 53u);
    double e = (double)(int64_t)(rnd64() >> (63 - sh)), A = (double)(int64_t)((rnd64() >> 40) * 256u);
    if (rnd64() & 1u) e = -e;
    if (rnd64() & 1u) A = -A;
    if (i % 7u == 0) A = (double)(int64_t)(rnd64() >> 11);  // and any integer up to 2^53
    if (i % 11u == 0) e = -A;                               // the sum is a zero
    if (!one(e, A)) return 1;
  }
  return 0;
}

int main() {
  unsigned long long scalings = 0, medians = 0, derivs = 0, partners = 0;
  if (check_scaling(&scalings) || check_median(&medians) || check_derivatives(&derivs) || check_partners(&partners)) return 1;
  std::printf("scalings %llu medians %llu derivatives %llu partners %llu ok\n", scalings, medians, derivs, partners);
  return 0;
}
