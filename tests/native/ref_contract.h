// ref_contract.h — the contract arithmetic that the scalar restatements (tests/native/*_ref.cpp) share, stated once.
// Like them it is built with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.  It includes nothing of the
// renderer's: the restatements stay independent of the code they check.  The fp32 -> fp16 rounding is written out here
// (h16), not taken from a library; tests/test_post_ref.py checks it against numpy over every case, and h2f and h16
// against each other over every half.  Every function is inline: a restatement uses the ones it needs.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

inline uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
inline float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// fp32 -> fp16, round to nearest even, on the bit patterns
inline uint16_t h16(float f) {
  const uint32_t u = bits(f), sign = (u >> 16) & 0x8000u, mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((mag >> 13) & 0x3ffu));  // NaN: quiet, payload's top bits
  if (mag >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to infinity (and infinity itself)
  if (mag < 0x33000000u) return (uint16_t)sign;               // < 2^-25: to zero (2^-25 itself ties to the even 0 below)
  const int e = (int)(mag >> 23) - 127;                       // unbiased exponent, -25 .. 15
  uint32_t m = (mag & 0x7fffffu) | 0x800000u;                 // 24-bit significand
  int shift;                                                  // bits dropped
  uint32_t base;
  if (e >= -14) {                                             // normal half: 10 fraction bits kept
    shift = 13;
    base = (uint32_t)(e + 15) << 10;
    m &= 0x7fffffu;
  } else {                                                    // subnormal half: value = m * 2^(e-23), unit 2^-24
    shift = -e - 1;                                           // 14 .. 24
    base = 0;
  }
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1u))) q++;           // a carry walks into the exponent, which is what it should do
  return (uint16_t)(sign | (base + q));
}

// fp16 -> fp32, exact
inline float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return from_bits(sign | 0x7f800000u | (m << 13));
  if (e != 0u) return from_bits(sign | ((e + 112u) << 23) | (m << 13));
  const float v = (float)m * 5.9604644775390625e-8f;  // m * 2^-24, exact
  return sign ? -v : v;
}

inline float san(float v) { return v > 0.0f ? (v < 65504.0f ? v : 65504.0f) : 0.0f; }
inline float sat(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }
inline uint32_t clampi(int64_t x, uint32_t n) { return x < 0 ? 0u : (x > (int64_t)n - 1 ? n - 1u : (uint32_t)x); }
inline int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// C41: the contract's 2^x
inline float exp2_poly(float x) {
  const float n = std::floor(x), f = x - n;
  float p = 0x1.ca8f0ap-13f;
  p = std::fma(p, f, 0x1.44d4d2p-10f);
  p = std::fma(p, f, 0x1.3d54d8p-7f);
  p = std::fma(p, f, 0x1.c67f5p-5f);
  p = std::fma(p, f, 0x1.ebfdf2p-3f);
  p = std::fma(p, f, 0x1.62e428p-1f);
  p = std::fma(p, f, 1.0f);
  return from_bits(bits(p) + ((uint32_t)(int32_t)n << 23));
}

// column-major matrix times (x, y, z, w), the C0 chain
inline void mat_vec(const float* m, float x, float y, float z, float w, float out[4]) {
  for (int r = 0; r < 4; r++) {
    float a = m[r] * x;
    a = std::fma(m[4 + r], y, a);
    a = std::fma(m[8 + r], z, a);
    a = std::fma(m[12 + r], w, a);
    out[r] = a;
  }
}

inline bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

// C17, up to the divide: the point (fx, fy) of the target, in pixels (a centre p + 0.5, or a corner), at depth z, as
// inv_viewproj gives it; kx = 2 / W, ky = 2 / H, divided once by the caller
inline void unproject(const float* inv_vp, float fx, float fy, float kx, float ky, float z, float h[4]) {
  mat_vec(inv_vp, std::fma(fx, kx, -1.0f), std::fma(fy, ky, -1.0f), z, 1.0f, h);
}
// C17's divide: one reciprocal of w, three products
inline void divide_w(const float h[4], float p[3]) {
  const float rw = 1.0f / h[3];
  for (int k = 0; k < 3; k++) p[k] = h[k] * rw;
}
// C17
inline void position(const float* inv_vp, float fx, float fy, float kx, float ky, float z, float p[3]) {
  float h[4];
  unproject(inv_vp, fx, fy, kx, ky, z, h);
  divide_w(h, p);
}

// C18's test of a homogeneous shadow-map position q against the nearest texel of a ws x hs map; half_w = ws / 2 and
// half_h = hs / 2, formed by the caller
inline bool shadow_test(const float q[4], float half_w, float half_h, uint32_t ws, uint32_t hs, float bias, const float* shadow) {
  const float rq = 1.0f / q[3];
  const float sx = std::fma(q[0] * rq, half_w, half_w), sy = std::fma(q[1] * rq, half_h, half_h);
  const float sz = q[2] * rq;
  const float fx = std::floor(sx), fy = std::floor(sy);
  return q[3] > 0.0f && fx >= 0.0f && fx < (float)ws && fy >= 0.0f && fy < (float)hs && sz + bias < shadow[(size_t)fy * ws + (size_t)fx];
}

// ---- C17-C19, one pixel: light_ref.cpp's, and ambient_ref.cpp's with the ambient factor
struct Light {
  float pos[3], radius, color[3], intensity;
};
struct LightFrame {  // the head of light_ref's <in>
  uint32_t W, H, n_lights, Ws, Hs;
  float inv_vp[16], ambient[4], sun_dir[4], sun_color[4], shadow_vp[16], bias;
};
static_assert(sizeof(LightFrame) == 5 * 4 + 45 * 4, "the input's head");

// the pixel (px, py) with depth z, normal nrm and albedo c -> its position p, whether the sun is shadowed there, and
// acc, which starts from fma(c * light, sun_color.w, c * ambient), the second product times *ao where ao is given
inline void light_pixel(const LightFrame& F, const Light* lights, const float* shadow, uint32_t px, uint32_t py, float z, const float* nrm,
                        const float* c, const float* ao, float p[3], bool& shadowed, float acc[3]) {
  // C17
  position(F.inv_vp, (float)px + 0.5f, (float)py + 0.5f, 2.0f / (float)F.W, 2.0f / (float)F.H, z, p);
  // C18
  const float d = std::fma(nrm[2], F.sun_dir[2], std::fma(nrm[1], F.sun_dir[1], nrm[0] * F.sun_dir[0]));
  shadowed = false;
  if (F.Ws) {
    float q[4];
    mat_vec(F.shadow_vp, p[0], p[1], p[2], 1.0f, q);
    shadowed = shadow_test(q, (float)F.Ws / 2.0f, (float)F.Hs / 2.0f, F.Ws, F.Hs, F.bias, shadow);
  }
  const float light = shadowed ? 0.1f : std::fmax(d, 0.1f);
  for (int ch = 0; ch < 3; ch++) acc[ch] = std::fma(c[ch] * light, F.sun_color[3], ao ? (c[ch] * F.ambient[ch]) * *ao : c[ch] * F.ambient[ch]);
  // C19
  for (uint32_t l = 0; l < F.n_lights; l++) {
    const Light& pl = lights[l];
    const float vx = pl.pos[0] - p[0], vy = pl.pos[1] - p[1], vz = pl.pos[2] - p[2];
    const float d2 = std::fma(vz, vz, std::fma(vy, vy, vx * vx));
    const float r2 = pl.radius * pl.radius;
    if (!(d2 < r2)) continue;
    const float ndl = std::fma(nrm[2], vz, std::fma(nrm[1], vy, nrm[0] * vx));
    if (!(ndl > 0.0f)) continue;
    const float t = 1.0f - d2 / r2;
    const float k = ((ndl / std::sqrt(d2)) * ((t * t) / (d2 + 1.0f))) * pl.intensity;
    for (int ch = 0; ch < 3; ch++) acc[ch] = std::fma(c[ch] * pl.color[ch], k, acc[ch]);
  }
}
