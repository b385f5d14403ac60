// motion_ref — scalar restatement of the camera motion blur pass's contract (include/svr_motion.h) for
// the tests: one pixel and one cell at a time, no tiles, no LDS.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one; `/` and std::sqrt are correctly
// rounded, std::rint rounds ties to even.  The fp32 -> fp16 rounding is written out (h16) in ref_contract.h.
//
//   motion_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, variant, 0; float reproject[16] (column-major), shutter, max_blur;
//       uint16 color[H][W][4] (fp16 bit patterns); float depth[H][W].
// <out>: uint16 color[H][W][4] after the pass; uint32 cw, ch; uint16 prepared[sh][sw][8] (san(rgb), 0, vx, vy, and the
//        depth's bits, low half first); uint64 M[ch][cw]; uint64 G[ch][cw]; float S[sh][sw], C72's sum of weights.
// variant 0 is the contract.  1 .. 9 are deliberately wrong (the tests check that each one is told apart):
//   1 the depth rule reversed            2 the tap's reach for every tap        3 the cover without the + 1
//   4 normalised by S, remainder dropped 5 G from the pixel's own cell only     6 16 taps always
//   7 the shutter not halved             8 vy negated                           9 reach from |v|, not the projection
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

struct Pass {
  uint32_t W, H, sx, sy, sw, sh, variant, pad;
  float reproject[16], shutter, max_blur;
};
static_assert(sizeof(Pass) == 8 * 4 + 18 * 4, "the input's head");

struct Texel {  // C68
  uint16_t rgb[3], vx, vy;
  float z;
};

bool fin(float v) { return std::fabs(v) < INFINITY; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: motion_ref <in> <out>\n");
    return 2;
  }
  Pass P;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  if (std::fread(&P, sizeof(P), 1, f) != 1) return 3;
  g_variant = (int)P.variant;
  if (P.sw == 0 || P.sh == 0 || P.sx + P.sw > P.W || P.sy + P.sh > P.H || !(P.max_blur >= 0.0f && P.max_blur <= 16.0f) || !(P.shutter >= 0.0f)) return 3;
  std::vector<uint16_t> color((size_t)P.W * P.H * 4);
  std::vector<float> depth((size_t)P.W * P.H);
  if (std::fread(color.data(), 2, color.size(), f) != color.size()) return 3;
  if (std::fread(depth.data(), 4, depth.size(), f) != depth.size()) return 3;
  std::fclose(f);
  const uint32_t sw = P.sw, sh = P.sh;

  // ---- C67, C68: the prepared image
  std::vector<Texel> prep((size_t)sw * sh);
  const float two_over_w = 2.0f / (float)P.W, two_over_h = 2.0f / (float)P.H;  // C17: divided once
  const float half_w = (float)P.W * 0.5f, half_h = (float)P.H * 0.5f;          // C29
  const float hs = g_variant == 7 ? P.shutter : 0.5f * P.shutter;
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++) {
      const uint32_t px = P.sx + x, py = P.sy + y;
      const size_t at = (size_t)py * P.W + px;
      const float z = depth[at];
      float q[4];
      mat_vec(P.reproject, std::fma((float)px + 0.5f, two_over_w, -1.0f), std::fma((float)py + 0.5f, two_over_h, -1.0f), z, 1.0f, q);
      const float r = 1.0f / q[3];
      const float hx = std::fma(q[0] * r, half_w, half_w), hy = std::fma(q[1] * r, half_h, half_h);
      float vx = (((float)px + 0.5f) - hx) * hs, vy = (((float)py + 0.5f) - hy) * hs;
      if (g_variant == 8) vy = -vy;
      if (!(q[3] > 0.0f) || !fin(vx) || !fin(vy)) vx = vy = 0.0f;
      const float l = std::sqrt(std::fma(vy, vy, vx * vx));
      if (l > P.max_blur) {
        const float k = P.max_blur / l;
        vx *= k;
        vy *= k;
      }
      Texel& t = prep[(size_t)y * sw + x];
      for (int j = 0; j < 3; j++) t.rgb[j] = h16(san(h2f(color[at * 4 + j])));
      t.vx = h16(vx);
      t.vy = h16(vy);
      t.z = z;
    }

  // ---- C69: cells, M and G
  const uint32_t cw = (sw + 7) / 8, ch = (sh + 7) / 8;
  std::vector<uint64_t> M((size_t)cw * ch, 0), G((size_t)cw * ch, 0);
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++) {
      const Texel& t = prep[(size_t)y * sw + x];
      const float vx = h2f(t.vx), vy = h2f(t.vy);
      const uint64_t key = ((uint64_t)bits(std::fma(vy, vy, vx * vx)) << 32) | ((uint32_t)t.vx << 16) | t.vy;
      uint64_t& m = M[(size_t)(y / 8) * cw + x / 8];
      m = key > m ? key : m;
    }
  const int Rc = g_variant == 5 ? 0 : ((int)std::ceil(P.max_blur) + 7) / 8;
  for (uint32_t cy = 0; cy < ch; cy++)
    for (uint32_t cx = 0; cx < cw; cx++) {
      uint64_t g = 0;
      for (int j = -Rc; j <= Rc; j++)
        for (int i = -Rc; i <= Rc; i++) {
          const uint64_t v = M[(size_t)clampi((int64_t)cy + j, ch) * cw + clampi((int64_t)cx + i, cw)];
          g = v > g ? v : g;
        }
      G[(size_t)cy * cw + cx] = g;
    }

  // ---- C70-C72: the gather
  std::vector<float> Ssum((size_t)sw * sh, 0.0f);
  const bool closed = P.shutter == 0.0f || P.max_blur == 0.0f;  // decided at the call, the target keeps its bits
  for (uint32_t y = 0; y < (closed ? 0u : sh); y++)
    for (uint32_t x = 0; x < sw; x++) {
      const uint64_t g = G[(size_t)(y / 8) * cw + x / 8];
      const float L2 = from_bits((uint32_t)(g >> 32));
      const float gx = h2f((uint16_t)(g >> 16)), gy = h2f((uint16_t)g);
      const Texel& own = prep[(size_t)y * sw + x];
      uint16_t* px = &color[((size_t)(P.sy + y) * P.W + P.sx + x) * 4];
      if (L2 < 0.25f) {
        for (int j = 0; j < 3; j++) px[j] = own.rgb[j];
        continue;
      }
      const int n = L2 > 64.0f && g_variant != 6 ? 32 : 16;
      const float rn = 1.0f / (float)n;
      const float rgl = 1.0f / std::sqrt(L2);
      // C71: a texel's reach along the dominant direction
      auto reach = [&](const Texel& t) {
        const float vx = h2f(t.vx), vy = h2f(t.vy);
        if (g_variant == 9) return std::sqrt(std::fma(vy, vy, vx * vx));
        return std::fabs(std::fma(vy, gy, vx * gx)) * rgl;
      };
      const float ep = reach(own);
      float acc[3] = {0.0f, 0.0f, 0.0f}, S = 0.0f;
      for (int k = 0; k < n; k++) {
        const float sa = (float)(2 * (k >> 1) + 1) * rn, s = (k & 1) ? -sa : sa;
        const int dx = (int)std::rint(gx * s), dy = (int)std::rint(gy * s);
        if (dx == 0 && dy == 0) continue;
        const float D = std::sqrt((float)(dx * dx + dy * dy));
        const Texel& t = prep[(size_t)clampi((int64_t)y + dy, sh) * sw + clampi((int64_t)x + dx, sw)];
        float e = (g_variant == 1 ? t.z > own.z : t.z < own.z) ? ep : reach(t);
        if (g_variant == 2) e = reach(t);
        const float w = g_variant == 3 ? sat(e - D) : sat((e - D) + 1.0f);
        for (int j = 0; j < 3; j++) acc[j] = std::fma(w, h2f(t.rgb[j]), acc[j]);
        S = S + w;
      }
      Ssum[(size_t)y * sw + x] = S;
      for (int j = 0; j < 3; j++) {
        if (g_variant == 4) px[j] = S > 0.0f ? h16(san(acc[j] / S)) : own.rgb[j];
        else px[j] = h16(san(std::fma((float)n - S, h2f(own.rgb[j]), acc[j]) * rn));
      }
    }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(color.data(), 2, color.size(), f);
  const uint32_t ext[2] = {cw, ch};
  std::fwrite(ext, 4, 2, f);
  for (const Texel& t : prep) {
    const uint32_t zb = bits(t.z);
    const uint16_t rec[8] = {t.rgb[0], t.rgb[1], t.rgb[2], 0, t.vx, t.vy, (uint16_t)zb, (uint16_t)(zb >> 16)};
    std::fwrite(rec, 2, 8, f);
  }
  std::fwrite(M.data(), 8, M.size(), f);
  std::fwrite(G.data(), 8, G.size(), f);
  std::fwrite(Ssum.data(), 4, Ssum.size(), f);
  return std::fclose(f) == 0 ? 0 : 4;
}
