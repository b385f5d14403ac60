// temporal_ref — scalar restatement of the temporal pass's contract (include/svr_temporal.h) for the
// tests: one pixel at a time, no tiles, every tap fetched where the contract says.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.  The fp32 -> fp16 rounding is
// ref_contract.h's, written out on the bit patterns (tests/test_post_ref.py pins it against numpy over every case).
//
//   temporal_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, flags, history_valid, variant; float reproject[16] (column-major),
//       blend; uint16 color[H][W][4] (fp16 bit patterns); float depth[H][W]; uint16 history[H][W][4].
// <out>: uint16 color[H][W][4] after the pass; uint16 history[H][W][4], the new history (zero outside the scissor);
//        uint8 valid[H][W], 1 where the pixel used the history.
// variant 0 is the contract.  1 .. 6 are deliberately wrong (the tests check that each one is told apart):
//   1 the smallest depth of the 3 x 3 instead of the largest   2 taps clamp to the target's edge, not the scissor's
//   3 the history sample sits at hx, not hx - 0.5               4 the clamp is applied after the blend
//   5 fma(blend, c - hc, hc) also when blend is 1               6 the history's lerp runs vertical first
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

float lerp(float t, float a, float b) { return std::fma(t, b - a, a); }

struct Pass {
  uint32_t W, H, sx, sy, sw, sh, flags, history_valid;
  float reproject[16], blend;
  std::vector<uint16_t> color, history;
  std::vector<float> depth;
};

// a coordinate clamped into the scissor (variant 2: into the target)
uint32_t cl(int64_t v, uint32_t lo, uint32_t n, uint32_t whole) {
  if (g_variant == 2) lo = 0, n = whole;
  return v < (int64_t)lo ? lo : (v > (int64_t)lo + n - 1 ? lo + n - 1u : (uint32_t)v);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  Pass P;
  uint32_t hdr[9];
  float par[17];
  if (std::fread(hdr, 4, 9, f) != 9 || std::fread(par, 4, 17, f) != 17) return 2;
  P.W = hdr[0]; P.H = hdr[1]; P.sx = hdr[2]; P.sy = hdr[3]; P.sw = hdr[4]; P.sh = hdr[5]; P.flags = hdr[6]; P.history_valid = hdr[7];
  g_variant = (int)hdr[8];
  std::memcpy(P.reproject, par, 64);
  P.blend = par[16];
  const size_t n = (size_t)P.W * P.H;
  P.color.resize(n * 4);
  P.depth.resize(n);
  P.history.resize(n * 4);
  if (std::fread(P.color.data(), 2, n * 4, f) != n * 4 || std::fread(P.depth.data(), 4, n, f) != n || std::fread(P.history.data(), 2, n * 4, f) != n * 4) return 2;
  std::fclose(f);
  if (P.sw == 0 || P.sh == 0 || P.sx + P.sw > P.W || P.sy + P.sh > P.H) return 2;

  std::vector<uint16_t> out_color = P.color, out_hist(n * 4, 0);
  std::vector<uint8_t> out_valid(n, 0);
  const float two_over_w = 2.0f / (float)P.W, two_over_h = 2.0f / (float)P.H;  // C17: divided once
  const float half_w = (float)P.W * 0.5f, half_h = (float)P.H * 0.5f;
  const float* m = P.reproject;
  const bool no_clamp = (P.flags & 2u) != 0u;
  for (uint32_t py = P.sy; py < P.sy + P.sh; py++)
    for (uint32_t px = P.sx; px < P.sx + P.sw; px++) {
      // C27, C28: the clamped 3 x 3
      float c[3], mn[3], mx[3], z = 0.0f;
      bool first = true;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const uint32_t x = cl((int64_t)px + dx, P.sx, P.sw, P.W), y = cl((int64_t)py + dy, P.sy, P.sh, P.H);
          const size_t at = (size_t)y * P.W + x;
          const float d = P.depth[at];
          for (int ch = 0; ch < 3; ch++) {
            const float v = san(h2f(P.color[at * 4 + ch]));
            if (first) mn[ch] = mx[ch] = v;
            mn[ch] = mn[ch] < v ? mn[ch] : v;
            mx[ch] = mx[ch] > v ? mx[ch] : v;
          }
          if (first) z = d;
          if (g_variant == 1) z = z < d ? z : d;
          else z = z > d ? z : d;
          first = false;
        }
      const size_t own = (size_t)py * P.W + px;
      for (int ch = 0; ch < 3; ch++) c[ch] = san(h2f(P.color[own * 4 + ch]));
      // C29 (not ref_contract.h's unproject: the chain runs over the x, y and w rows only, z is never formed)
      const float xn = std::fma((float)px + 0.5f, two_over_w, -1.0f), yn = std::fma((float)py + 0.5f, two_over_h, -1.0f);
      float qx = m[0] * xn, qy = m[1] * xn, qw = m[3] * xn;
      qx = std::fma(m[4], yn, qx); qy = std::fma(m[5], yn, qy); qw = std::fma(m[7], yn, qw);
      qx = std::fma(m[8], z, qx); qy = std::fma(m[9], z, qy); qw = std::fma(m[11], z, qw);
      qx = std::fma(m[12], 1.0f, qx); qy = std::fma(m[13], 1.0f, qy); qw = std::fma(m[15], 1.0f, qw);
      bool valid = P.history_valid != 0u && qw > 0.0f;
      float hist[3] = {0.0f, 0.0f, 0.0f};
      if (valid) {
        const float r = 1.0f / qw;
        const float hx = std::fma(qx * r, half_w, half_w), hy = std::fma(qy * r, half_h, half_h);
        valid = hx >= (float)P.sx && hx < (float)(P.sx + P.sw) && hy >= (float)P.sy && hy < (float)(P.sy + P.sh);
        if (valid) {
          // C30
          const float fx = g_variant == 3 ? hx : hx - 0.5f, fy = g_variant == 3 ? hy : hy - 0.5f;
          const float flx = std::floor(fx), fly = std::floor(fy);
          const float tx = fx - flx, ty = fy - fly;
          const uint32_t x0 = cl((int64_t)flx, P.sx, P.sw, P.W), x1 = cl((int64_t)flx + 1, P.sx, P.sw, P.W);
          const uint32_t y0 = cl((int64_t)fly, P.sy, P.sh, P.H), y1 = cl((int64_t)fly + 1, P.sy, P.sh, P.H);
          for (int ch = 0; ch < 3; ch++) {
            const float a = h2f(P.history[((size_t)y0 * P.W + x0) * 4 + ch]), b = h2f(P.history[((size_t)y0 * P.W + x1) * 4 + ch]);
            const float cc = h2f(P.history[((size_t)y1 * P.W + x0) * 4 + ch]), d = h2f(P.history[((size_t)y1 * P.W + x1) * 4 + ch]);
            if (g_variant == 6) hist[ch] = lerp(tx, lerp(ty, a, cc), lerp(ty, b, d));
            else hist[ch] = lerp(ty, lerp(tx, a, b), lerp(tx, cc, d));
          }
        }
      }
      // C31
      for (int ch = 0; ch < 3; ch++) {
        float hc = hist[ch];
        if (!no_clamp && g_variant != 4) {
          hc = hc < mn[ch] ? mn[ch] : hc;
          hc = hc > mx[ch] ? mx[ch] : hc;
        }
        float o = (valid && (P.blend < 1.0f || g_variant == 5)) ? std::fma(P.blend, c[ch] - hc, hc) : c[ch];
        if (!no_clamp && g_variant == 4 && valid && P.blend < 1.0f) {
          o = o < mn[ch] ? mn[ch] : o;
          o = o > mx[ch] ? mx[ch] : o;
        }
        const uint16_t hb = h16(o);
        out_hist[own * 4 + ch] = hb;
        out_color[own * 4 + ch] = hb;
      }
      out_valid[own] = valid ? 1 : 0;
    }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out_color.data(), 2, n * 4, f);
  std::fwrite(out_hist.data(), 2, n * 4, f);
  std::fwrite(out_valid.data(), 1, n, f);
  std::fclose(f);
  return 0;
}
