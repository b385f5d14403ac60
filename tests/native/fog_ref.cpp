// fog_ref — scalar restatement of the fog pass's contract (include/svr_fog.h) for the tests: one block
// and one pixel at a time, no tiles, no LDS.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one; `/` and std::sqrt are correctly
// rounded.  The fp32 -> fp16 rounding is written out (h16) in ref_contract.h, with C17, C18's test and C41.
//
//   fog_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, steps, frame_index, shadow_w, shadow_h (0, 0: no map), variant,
//       pin (1: every block's dither o is pin_o);
//       float inv_viewproj[16], camera[3], density, height_falloff, height_base, max_distance, fog_color[3], anisotropy,
//       sunlight_direction[4], sun_color[3], edge_sharpness, shadow_viewproj[16], shadow_bias, pin_o;
//       uint16 color[H][W][4] (fp16 bit patterns); float depth[H][W]; float shadow[shadow_h][shadow_w].
// <out>: uint16 color[H][W][4] after the pass; uint32 gw, gh; float st[gh][gw][4] (S.rgb, T); float t_end[gh][gw].
// variant 0 is the contract.  1 .. 9 are deliberately wrong (the tests check that each one is told apart):
//   1 T is updated before S          2 no dither: o = 1/2 everywhere       3 the sample sits at the step's start
//   4 plain bilinear upsample        5 the bias is subtracted              6 height is measured from the camera
//   7 g is negated                   8 a block is marched to its nearest pixel     9 the taps' upper clamp is off by one
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

float into(float x, float lo, float hi) {
  x = x > lo ? x : lo;
  return x < hi ? x : hi;
}

struct Pass {
  uint32_t W, H, sx, sy, sw, sh, steps, frame, shadow_w, shadow_h, variant, pin;
  float inv_viewproj[16], cam[3], density, falloff, base, max_distance, fog[3], g, sun_dir[4], sun_color[3], edge, shadow_viewproj[16], bias, pin_o;
};
static_assert(sizeof(Pass) == 12 * 4 + 53 * 4, "the input's head");

Pass P;
std::vector<float> depth, shadow;
float two_over_w, two_over_h;

// C55: t(pixel)
float pixel_t(uint32_t x, uint32_t y) {
  const float z = depth[(size_t)y * P.W + x];
  if (bits(z) == 0u) return P.max_distance;
  float p[3];
  position(P.inv_viewproj, (float)x + 0.5f, (float)y + 0.5f, two_over_w, two_over_h, z, p);
  const float vx = p[0] - P.cam[0], vy = p[1] - P.cam[1], vz = p[2] - P.cam[2];
  const float t = std::sqrt(std::fma(vz, vz, std::fma(vy, vy, vx * vx)));
  return t < P.max_distance ? t : P.max_distance;
}

// C56
uint32_t fog_hash(uint32_t bx, uint32_t by, uint32_t frame) {
  uint32_t h = (bx * 0x9E3779B1u) ^ (by * 0x85EBCA77u) ^ (frame * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: fog_ref <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  if (std::fread(&P, sizeof(P), 1, f) != 1) return 3;
  g_variant = (int)P.variant;
  if (P.sw == 0 || P.sh == 0 || P.sx + P.sw > P.W || P.sy + P.sh > P.H || P.steps < 1 || P.steps > 64) return 3;
  std::vector<uint16_t> color((size_t)P.W * P.H * 4);
  depth.resize((size_t)P.W * P.H);
  shadow.resize((size_t)P.shadow_w * P.shadow_h);
  if (std::fread(color.data(), 2, color.size(), f) != color.size()) return 3;
  if (std::fread(depth.data(), 4, depth.size(), f) != depth.size()) return 3;
  if (!shadow.empty() && std::fread(shadow.data(), 4, shadow.size(), f) != shadow.size()) return 3;
  std::fclose(f);
  const bool has_map = !shadow.empty();

  // what the call computes once
  const float LOG2E = 0x1.715476p+0f, FOUR_PI = 0x1.921fb6p+3f;
  two_over_w = 2.0f / (float)P.W;
  two_over_h = 2.0f / (float)P.H;
  const float kh = P.falloff * LOG2E;
  float sun[3];
  {
    const float* L = P.sun_dir;
    const float l2 = std::fma(L[2], L[2], std::fma(L[1], L[1], L[0] * L[0]));
    const bool ok = std::isfinite(l2) && l2 > 0.0f;
    const float inv = ok ? 1.0f / std::sqrt(l2) : 0.0f;
    for (int k = 0; k < 3; k++) sun[k] = ok ? L[k] * inv : 0.0f;
  }
  const float g = g_variant == 7 ? -P.g : P.g, g2 = g * g;
  const float one_plus_g2 = 1.0f + g2, minus_2g = -2.0f * g, one_minus_g2 = 1.0f - g2;
  const float half_w = (float)P.shadow_w * 0.5f, half_h = (float)P.shadow_h * 0.5f;
  const float bias = g_variant == 5 ? -P.bias : P.bias;
  const float base = g_variant == 6 ? P.cam[1] : P.base;

  // ---- C55-C58: the half-resolution march
  const uint32_t gw = (P.sw + 1) / 2, gh = (P.sh + 1) / 2;
  std::vector<float> st((size_t)gw * gh * 4), te((size_t)gw * gh);
  for (uint32_t by = 0; by < gh; by++)
    for (uint32_t bx = 0; bx < gw; bx++) {
      const uint32_t x0 = P.sx + 2 * bx, y0 = P.sy + 2 * by;
      const bool two_x = 2 * bx + 1 < P.sw, two_y = 2 * by + 1 < P.sh;
      float m = pixel_t(x0, y0);
      auto take = [&](float v) { m = g_variant == 8 ? (v < m ? v : m) : (v > m ? v : m); };
      if (two_x) take(pixel_t(x0 + 1, y0));
      if (two_y) {
        take(pixel_t(x0, y0 + 1));
        if (two_x) take(pixel_t(x0 + 1, y0 + 1));
      }
      const float t_end = m;
      float d[3];
      {
        float p[3];  // C17 at the block's middle, a pixel corner, on the near plane
        position(P.inv_viewproj, (float)x0 + 1.0f, (float)y0 + 1.0f, two_over_w, two_over_h, 1.0f, p);
        const float vx = p[0] - P.cam[0], vy = p[1] - P.cam[1], vz = p[2] - P.cam[2];
        const float inv = 1.0f / std::sqrt(std::fma(vz, vz, std::fma(vy, vy, vx * vx)));
        d[0] = vx * inv; d[1] = vy * inv; d[2] = vz * inv;
      }
      const float delta = t_end / (float)P.steps;
      float o = (float)(fog_hash(bx, by, P.frame) >> 24) * 0x1p-8f;
      if (P.pin) o = P.pin_o;
      if (g_variant == 2) o = 0.5f;
      if (g_variant == 3) o = 0.0f;
      const float c = std::fma(d[2], sun[2], std::fma(d[1], sun[1], d[0] * sun[0]));
      const float x = std::fma(minus_2g, c, one_plus_g2);
      const float ph = one_minus_g2 / (FOUR_PI * (x * std::sqrt(x)));
      float lit[3], dark[3];
      for (int k = 0; k < 3; k++) {
        lit[k] = std::fma(P.sun_color[k], ph, P.fog[k]);
        dark[k] = std::fma(P.sun_color[k], 0.0f, P.fog[k]);
      }
      float q0[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
      if (has_map) {
        const float* M = P.shadow_viewproj;
        mat_vec(M, P.cam[0], P.cam[1], P.cam[2], 1.0f, q0);
        for (int k = 0; k < 4; k++) dq[k] = std::fma(M[8 + k], d[2], std::fma(M[4 + k], d[1], M[k] * d[0]));
      }
      float S[3] = {0.0f, 0.0f, 0.0f}, T = 1.0f;
      for (uint32_t i = 0; i < P.steps; i++) {
        const float ti = ((float)i + o) * delta;
        const float yi = std::fma(ti, d[1], P.cam[1]);
        const float sigma = P.density * exp2_poly(into((base - yi) * kh, -16.0f, 16.0f));
        const float a = exp2_poly(into((sigma * delta) * -LOG2E, -16.0f, 0.0f));
        bool shadowed = false;
        if (has_map) {
          float q[4];
          for (int k = 0; k < 4; k++) q[k] = std::fma(ti, dq[k], q0[k]);
          shadowed = shadow_test(q, half_w, half_h, P.shadow_w, P.shadow_h, bias, shadow.data());
        }
        if (g_variant == 1) T = T * a;
        const float w = T * (1.0f - a);
        for (int k = 0; k < 3; k++) S[k] = std::fma(w, shadowed ? dark[k] : lit[k], S[k]);
        if (g_variant != 1) T = T * a;
      }
      const size_t at = (size_t)by * gw + bx;
      st[at * 4 + 0] = S[0]; st[at * 4 + 1] = S[1]; st[at * 4 + 2] = S[2]; st[at * 4 + 3] = T;
      te[at] = t_end;
    }

  // ---- C59, C60: upsample and composite
  const uint32_t cw = g_variant == 9 && gw > 1 ? gw - 1 : gw, ch = g_variant == 9 && gh > 1 ? gh - 1 : gh;
  // (density == 0: decided at the call, the target keeps its bits)
  for (uint32_t y = 0; y < (P.density == 0.0f ? 0u : P.sh); y++)
    for (uint32_t x = 0; x < P.sw; x++) {
      const float tp = pixel_t(P.sx + x, P.sy + y);
      const float u = std::fma((float)x, 0.5f, -0.25f), v = std::fma((float)y, 0.5f, -0.25f);
      const float flx = std::floor(u), fly = std::floor(v);
      const float tx = u - flx, ty = v - fly;
      const uint32_t xs[2] = {clampi((int64_t)flx, cw), clampi((int64_t)flx + 1, cw)};
      const uint32_t ys[2] = {clampi((int64_t)fly, ch), clampi((int64_t)fly + 1, ch)};
      const float b[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
      float num[4] = {0, 0, 0, 0}, den = 0.0f;
      for (int k = 0; k < 4; k++) {
        const size_t at = (size_t)ys[k >> 1] * gw + xs[k & 1];
        const float w = g_variant == 4 ? b[k] : b[k] / std::fma(P.edge, std::fabs(te[at] - tp), 1.0f);
        for (int j = 0; j < 4; j++) num[j] = k == 0 ? w * st[at * 4 + j] : std::fma(w, st[at * 4 + j], num[j]);
        den = k == 0 ? w : den + w;
      }
      const float rd = 1.0f / den;
      const float T = num[3] * rd;
      uint16_t* px = &color[((size_t)(P.sy + y) * P.W + P.sx + x) * 4];
      for (int j = 0; j < 3; j++) px[j] = h16(san(std::fma(h2f(px[j]), T, num[j] * rd)));
    }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(color.data(), 2, color.size(), f);
  const uint32_t ext[2] = {gw, gh};
  std::fwrite(ext, 4, 2, f);
  std::fwrite(st.data(), 4, st.size(), f);
  std::fwrite(te.data(), 4, te.size(), f);
  return std::fclose(f) == 0 ? 0 : 4;
}
