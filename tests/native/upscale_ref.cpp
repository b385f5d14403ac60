// upscale_ref — scalar restatement of the upscaled present's contract (include/svr_upscale.h) for the
// tests: one output texel at a time, no tiles, no tables.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.
//
//   upscale_ref <in> <out> [<floats>]
// <in>  (little endian): uint32 W, H, dw, dh, src_format (0 RGBA16F, 1 RGBA8), dst_format (0 B8G8R8A8, 1 R8G8B8A8), flags,
//       variant; float sharpness; then the colour target: uint16 [H][W][4] (fp16 bit patterns) or uint8 [H][W][4].
// <out>: uint8 [dh][dw][4], the destination's bytes.  <floats>, if named: float [dh][dw][4], the values before un8 (R, G, B, A).
// variant 0 is the contract.  1 .. 6 are deliberately wrong (the tests check that each one is told apart):
//   1 the taps' upper clamp is off by one        2 w0 and w3 are swapped               3 columns are filtered before rows
//   4 the anti-ringing clamp is missing          5 the sharpen reads quantised neighbours
//   6 the sharpen's neighbours are not clamped at the image border (P is evaluated outside the image instead)
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;
uint32_t W, H, DW, DH;
float g_su, g_sv;
std::vector<float> g_src;  // [H][W][4], decoded and saturated (C50)

float lo2(float a, float b) { return a < b ? a : b; }
float hi2(float a, float b) { return a > b ? a : b; }
uint32_t un8(float f) { return (uint32_t)(int)std::rint(lo2(hi2(f, 0.0f), 1.0f) * 255.0f); }  // round to nearest even

// C50
float s(int x, int y, int ch) {
  const int xmax = g_variant == 1 ? (W > 1u ? (int)W - 2 : 0) : (int)W - 1, ymax = g_variant == 1 ? (H > 1u ? (int)H - 2 : 0) : (int)H - 1;
  x = x < 0 ? 0 : (x > xmax ? xmax : x);
  y = y < 0 ? 0 : (y > ymax ? ymax : y);
  return g_src[((size_t)y * W + (size_t)x) * 4 + ch];
}

// C51, C52: the first central tap and the four weights of output index i
struct Axis {
  int x0;
  float w[4];
};
Axis axis(int i, float scale) {
  const float u = ((float)i + 0.5f) * scale - 0.5f;
  const float f = std::floor(u);
  const float t = u - f;
  Axis a;
  a.x0 = (int)f;
  a.w[0] = std::fma(std::fma(-0.5f, t, 1.0f), t, -0.5f) * t;
  a.w[1] = std::fma(std::fma(1.5f, t, -2.5f), t * t, 1.0f);
  a.w[2] = std::fma(std::fma(-1.5f, t, 2.0f), t, 0.5f) * t;
  a.w[3] = std::fma(0.5f, t, -0.5f) * (t * t);
  if (g_variant == 2) {
    const float k = a.w[0];
    a.w[0] = a.w[3];
    a.w[3] = k;
  }
  return a;
}
float filter4(const float* w, float s0, float s1, float s2, float s3) { return std::fma(w[3], s3, std::fma(w[2], s2, std::fma(w[1], s1, w[0] * s0))); }

// C52: P of output (i, j), channel ch
float P(int i, int j, int ch) {
  const Axis ax = axis(i, g_su), ay = axis(j, g_sv);
  float r[4];
  if (g_variant == 3) {
    for (int k = 0; k < 4; k++) r[k] = filter4(ay.w, s(ax.x0 - 1 + k, ay.x0 - 1, ch), s(ax.x0 - 1 + k, ay.x0, ch), s(ax.x0 - 1 + k, ay.x0 + 1, ch), s(ax.x0 - 1 + k, ay.x0 + 2, ch));
  } else {
    for (int k = 0; k < 4; k++) r[k] = filter4(ax.w, s(ax.x0 - 1, ay.x0 - 1 + k, ch), s(ax.x0, ay.x0 - 1 + k, ch), s(ax.x0 + 1, ay.x0 - 1 + k, ch), s(ax.x0 + 2, ay.x0 - 1 + k, ch));
  }
  const float p = filter4(g_variant == 3 ? ax.w : ay.w, r[0], r[1], r[2], r[3]);
  if (g_variant == 4) return p;
  const float c00 = s(ax.x0, ay.x0, ch), c10 = s(ax.x0 + 1, ay.x0, ch), c01 = s(ax.x0, ay.x0 + 1, ch), c11 = s(ax.x0 + 1, ay.x0 + 1, ch);
  const float lo = lo2(lo2(c00, c10), lo2(c01, c11)), hi = hi2(hi2(c00, c10), hi2(c01, c11));
  return lo2(hi2(p, lo), hi);
}

// a neighbour of the sharpen
float neighbour(int i, int j, int ch) {
  if (g_variant != 6) {
    i = i < 0 ? 0 : (i > (int)DW - 1 ? (int)DW - 1 : i);
    j = j < 0 ? 0 : (j > (int)DH - 1 ? (int)DH - 1 : j);
  }
  const float p = P(i, j, ch);
  return g_variant == 5 ? (float)un8(p) * 0x1.010102p-8f : p;
}

// C53
float sharpen(int i, int j, int ch, float peak) {
  const float m = P(i, j, ch), n = neighbour(i, j - 1, ch), so = neighbour(i, j + 1, ch), e = neighbour(i + 1, j, ch), w = neighbour(i - 1, j, ch);
  const float lo = lo2(lo2(lo2(n, so), lo2(e, w)), m), hi = hi2(hi2(hi2(n, so), hi2(e, w)), m);
  const float a = hi > 0.0f ? lo2(lo, 1.0f - hi) / hi : 0.0f;
  const float k = a * peak;
  return std::fma(k, (n + so) + (e + w), m) / std::fma(4.0f, k, 1.0f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[8];
  float sharpness;
  if (std::fread(hdr, 4, 8, f) != 8 || std::fread(&sharpness, 4, 1, f) != 1) return 2;
  W = hdr[0];
  H = hdr[1];
  DW = hdr[2];
  DH = hdr[3];
  const uint32_t src_fmt = hdr[4], dst_fmt = hdr[5], flags = hdr[6];
  g_variant = (int)hdr[7];
  if (W == 0 || H == 0 || DW < W || DH < H || src_fmt > 1 || dst_fmt > 1) return 2;
  const size_t n = (size_t)W * H * 4;
  g_src.resize(n);
  if (src_fmt == 0) {
    std::vector<uint16_t> raw(n);
    if (std::fread(raw.data(), 2, n, f) != n) return 2;
    for (size_t i = 0; i < n; i++) g_src[i] = sat(h2f(raw[i]));
  } else {
    std::vector<uint8_t> raw(n);
    if (std::fread(raw.data(), 1, n, f) != n) return 2;
    for (size_t i = 0; i < n; i++) g_src[i] = sat((float)raw[i] * 0x1.010102p-8f);
  }
  std::fclose(f);
  g_su = (float)W / (float)DW;
  g_sv = (float)H / (float)DH;
  const float peak = -1.0f / (8.0f - 3.0f * sharpness);
  const bool sharp = !(flags & 1u);
  std::vector<uint8_t> out((size_t)DW * DH * 4);
  std::vector<float> values((size_t)DW * DH * 4);
  for (uint32_t j = 0; j < DH; j++)
    for (uint32_t i = 0; i < DW; i++) {
      uint32_t q[4];
      for (int ch = 0; ch < 4; ch++) {
        const float v = sharp && ch < 3 ? sharpen((int)i, (int)j, ch, peak) : P((int)i, (int)j, ch);
        values[((size_t)j * DW + i) * 4 + ch] = v;
        q[ch] = un8(v);
      }
      uint8_t* o = &out[((size_t)j * DW + i) * 4];
      o[0] = (uint8_t)(dst_fmt == 0 ? q[2] : q[0]);  // C54: B8G8R8A8 stores blue first
      o[1] = (uint8_t)q[1];
      o[2] = (uint8_t)(dst_fmt == 0 ? q[0] : q[2]);
      o[3] = (uint8_t)q[3];
    }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
  std::fclose(f);
  if (argc == 4) {
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(values.data(), 4, values.size(), f) != values.size()) return 2;
    std::fclose(f);
  }
  return 0;
}
