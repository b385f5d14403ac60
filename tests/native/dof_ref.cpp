// dof_ref — scalar restatement of the depth of field pass's contract (include/svr_dof.h) for the tests:
// one pixel and one cell at a time, no tiles, no LDS.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one; `/` and std::sqrt are correctly
// rounded, std::rint rounds ties to even.  The fp32 -> fp16 rounding is written out (h16) in ref_contract.h.
//
//   dof_ref <in> <out>
//   dof_ref --taps          prints the tap table below, one tap per line: the bit patterns of x and y in hex
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, variant, 0;
//       float inv_z_scale, inv_z_bias, focus_distance, blur_scale, max_radius;
//       uint16 color[H][W][4] (fp16 bit patterns); float depth[H][W].
// <out>: uint16 color[H][W][4] after the pass; uint32 cw, ch; uint16 prepared[sh][sw][4] (san(rgb), c);
//        float M[ch][cw]; float g[ch][cw].
// variant 0 is the contract.  1 .. 12 are deliberately wrong (the tests check that each one is told apart):
//   1 the sign of c flipped               2 e_k = |c_k| whatever lies behind   3 the cover without the + 1
//   4 1 / e instead of 1 / e^2            5 the centre tap left out            6 zero-offset taps counted
//   7 the cell reach one cell short       8 M taken over the 32 x 16 tile      9 the taps' upper clamp off by one
//  10 dist from the clamped offsets      11 the even ring not turned          12 r clamped from above only
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

// C64: the taps, as csrc/svr_dof_taps.h holds them (tests/test_dof_ref.py regenerates them from the formula)
const float TAPS[49][2] = {
    {0x0.0p+0f, 0x0.0p+0f},
    {0x1.555556p-2f, 0x0.0p+0f},
    {0x1.e2b7dep-3f, 0x1.e2b7dep-3f},
    {0x0.0p+0f, 0x1.555556p-2f},
    {-0x1.e2b7dep-3f, 0x1.e2b7dep-3f},
    {-0x1.555556p-2f, 0x0.0p+0f},
    {-0x1.e2b7dep-3f, -0x1.e2b7dep-3f},
    {0x0.0p+0f, -0x1.555556p-2f},
    {0x1.e2b7dep-3f, -0x1.e2b7dep-3f},
    {0x1.4ec654p-1f, 0x1.0a5d02p-3f},
    {0x1.1bceecp-1f, 0x1.7b44fp-2f},
    {0x1.7b44fp-2f, 0x1.1bceecp-1f},
    {0x1.0a5d02p-3f, 0x1.4ec654p-1f},
    {-0x1.0a5d02p-3f, 0x1.4ec654p-1f},
    {-0x1.7b44fp-2f, 0x1.1bceecp-1f},
    {-0x1.1bceecp-1f, 0x1.7b44fp-2f},
    {-0x1.4ec654p-1f, 0x1.0a5d02p-3f},
    {-0x1.4ec654p-1f, -0x1.0a5d02p-3f},
    {-0x1.1bceecp-1f, -0x1.7b44fp-2f},
    {-0x1.7b44fp-2f, -0x1.1bceecp-1f},
    {-0x1.0a5d02p-3f, -0x1.4ec654p-1f},
    {0x1.0a5d02p-3f, -0x1.4ec654p-1f},
    {0x1.7b44fp-2f, -0x1.1bceecp-1f},
    {0x1.1bceecp-1f, -0x1.7b44fp-2f},
    {0x1.4ec654p-1f, -0x1.0a5d02p-3f},
    {0x1.0p+0f, 0x0.0p+0f},
    {0x1.ee8dd4p-1f, 0x1.0907dcp-2f},
    {0x1.bb67aep-1f, 0x1.0p-1f},
    {0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
    {0x1.0p-1f, 0x1.bb67aep-1f},
    {0x1.0907dcp-2f, 0x1.ee8dd4p-1f},
    {0x0.0p+0f, 0x1.0p+0f},
    {-0x1.0907dcp-2f, 0x1.ee8dd4p-1f},
    {-0x1.0p-1f, 0x1.bb67aep-1f},
    {-0x1.6a09e6p-1f, 0x1.6a09e6p-1f},
    {-0x1.bb67aep-1f, 0x1.0p-1f},
    {-0x1.ee8dd4p-1f, 0x1.0907dcp-2f},
    {-0x1.0p+0f, 0x0.0p+0f},
    {-0x1.ee8dd4p-1f, -0x1.0907dcp-2f},
    {-0x1.bb67aep-1f, -0x1.0p-1f},
    {-0x1.6a09e6p-1f, -0x1.6a09e6p-1f},
    {-0x1.0p-1f, -0x1.bb67aep-1f},
    {-0x1.0907dcp-2f, -0x1.ee8dd4p-1f},
    {0x0.0p+0f, -0x1.0p+0f},
    {0x1.0907dcp-2f, -0x1.ee8dd4p-1f},
    {0x1.0p-1f, -0x1.bb67aep-1f},
    {0x1.6a09e6p-1f, -0x1.6a09e6p-1f},
    {0x1.bb67aep-1f, -0x1.0p-1f},
    {0x1.ee8dd4p-1f, -0x1.0907dcp-2f},
};

struct Pass {
  uint32_t W, H, sx, sy, sw, sh, variant, pad;
  float inv_z_scale, inv_z_bias, focus, blur_scale, max_radius;
};
static_assert(sizeof(Pass) == 8 * 4 + 5 * 4, "the input's head");

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "--taps") == 0) {
    for (int k = 0; k < 49; k++) std::printf("%08x %08x\n", bits(TAPS[k][0]), bits(TAPS[k][1]));
    return 0;
  }
  if (argc != 3) {
    std::fprintf(stderr, "usage: dof_ref <in> <out> | dof_ref --taps\n");
    return 2;
  }
  Pass P;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  if (std::fread(&P, sizeof(P), 1, f) != 1) return 3;
  g_variant = (int)P.variant;
  if (P.sw == 0 || P.sh == 0 || P.sx + P.sw > P.W || P.sy + P.sh > P.H || !(P.max_radius >= 0.0f && P.max_radius <= 16.0f)) return 3;
  std::vector<uint16_t> color((size_t)P.W * P.H * 4);
  std::vector<float> depth((size_t)P.W * P.H);
  if (std::fread(color.data(), 2, color.size(), f) != color.size()) return 3;
  if (std::fread(depth.data(), 4, depth.size(), f) != depth.size()) return 3;
  std::fclose(f);
  const uint32_t sw = P.sw, sh = P.sh;

  // ---- C61, C62: the prepared image
  std::vector<uint16_t> prep((size_t)sw * sh * 4);
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++) {
      const size_t at = (size_t)(P.sy + y) * P.W + P.sx + x;
      const float iz = std::fma(depth[at], P.inv_z_scale, P.inv_z_bias);
      float r = P.blur_scale * std::fma(-P.focus, iz, 1.0f);
      if (g_variant == 1) r = -r;
      r = r == r ? r : 0.0f;
      if (g_variant != 12) r = r > -P.max_radius ? r : -P.max_radius;
      r = r < P.max_radius ? r : P.max_radius;
      uint16_t* q = &prep[((size_t)y * sw + x) * 4];
      for (int j = 0; j < 3; j++) q[j] = h16(san(h2f(color[at * 4 + j])));
      q[3] = h16(r);
    }

  // ---- C63: cells, M and g
  const uint32_t cw = (sw + 7) / 8, ch = (sh + 7) / 8;
  std::vector<float> M((size_t)cw * ch, 0.0f), G((size_t)cw * ch, 0.0f);
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++) {
      const float a = std::fabs(h2f(prep[((size_t)y * sw + x) * 4 + 3]));
      float& m = M[(size_t)(y / 8) * cw + x / 8];
      m = a > m ? a : m;
    }
  const int R = (int)std::ceil(P.max_radius);
  int Rc = (R + 7) / 8;
  if (g_variant == 7) Rc -= 1;
  for (uint32_t cy = 0; cy < ch; cy++)
    for (uint32_t cx = 0; cx < cw; cx++) {
      float g = 0.0f;
      if (g_variant == 8) {  // the cells of the pixel's 32 x 16 tile instead
        for (uint32_t j = cy / 2 * 2; j < cy / 2 * 2 + 2 && j < ch; j++)
          for (uint32_t i = cx / 4 * 4; i < cx / 4 * 4 + 4 && i < cw; i++) g = M[(size_t)j * cw + i] > g ? M[(size_t)j * cw + i] : g;
      } else {
        for (int j = -Rc; j <= Rc; j++)
          for (int i = -Rc; i <= Rc; i++) {
            const float v = M[(size_t)clampi((int64_t)cy + j, ch) * cw + clampi((int64_t)cx + i, cw)];
            g = v > g ? v : g;
          }
      }
      G[(size_t)cy * cw + cx] = g;
    }

  // ---- C64-C66: the gather
  float taps[49][2];
  std::memcpy(taps, TAPS, sizeof(taps));
  if (g_variant == 11)
    for (int i = 0; i < 16; i++) {
      const double a = (2.0 * 3.14159265358979323846) * i / 16.0;
      taps[9 + i][0] = (float)((2.0 / 3.0) * std::cos(a));
      taps[9 + i][1] = (float)((2.0 / 3.0) * std::sin(a));
    }
  const uint32_t clamp_w = g_variant == 9 && sw > 1 ? sw - 1 : sw, clamp_h = g_variant == 9 && sh > 1 ? sh - 1 : sh;
  const bool pinhole = P.blur_scale == 0.0f || P.max_radius == 0.0f;  // decided at the call, the target keeps its bits
  for (uint32_t y = 0; y < (pinhole ? 0u : sh); y++)
    for (uint32_t x = 0; x < sw; x++) {
      const float g = G[(size_t)(y / 8) * cw + x / 8];
      const float cp = h2f(prep[((size_t)y * sw + x) * 4 + 3]), acp = std::fabs(cp);
      float acc[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
      for (int k = g_variant == 5 ? 1 : 0; k < 49; k++) {
        const int dx = (int)std::rint(taps[k][0] * g), dy = (int)std::rint(taps[k][1] * g);
        if (k != 0 && dx == 0 && dy == 0 && g_variant != 6) continue;
        const uint32_t tx = clampi((int64_t)x + dx, clamp_w), ty = clampi((int64_t)y + dy, clamp_h);
        int ddx = dx, ddy = dy;
        if (g_variant == 10) {
          ddx = (int)tx - (int)x;
          ddy = (int)ty - (int)y;
        }
        const float dist = std::sqrt((float)(ddx * ddx + ddy * ddy));
        const uint16_t* q = &prep[((size_t)ty * sw + tx) * 4];
        const float ck = h2f(q[3]), ack = std::fabs(ck);
        float e = ck > cp ? (ack < acp ? ack : acp) : ack;
        if (g_variant == 2) e = ack;
        const float e2 = g_variant == 4 ? e : e * e;
        const float cover = g_variant == 3 ? sat(e - dist) : sat((e - dist) + 1.0f);
        const float w = cover / (e2 > 1.0f ? e2 : 1.0f);
        for (int j = 0; j < 3; j++) acc[j] = std::fma(w, h2f(q[j]), acc[j]);
        W = W + w;
      }
      uint16_t* px = &color[((size_t)(P.sy + y) * P.W + P.sx + x) * 4];
      for (int j = 0; j < 3; j++) px[j] = h16(san(acc[j] / W));
    }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(color.data(), 2, color.size(), f);
  const uint32_t ext[2] = {cw, ch};
  std::fwrite(ext, 4, 2, f);
  std::fwrite(prep.data(), 2, prep.size(), f);
  std::fwrite(M.data(), 4, M.size(), f);
  std::fwrite(G.data(), 4, G.size(), f);
  return std::fclose(f) == 0 ? 0 : 4;
}
