// post_ref — scalar restatement of the post pass's contract (include/svr_post.h) for the tests: whole
// level images, one texel at a time, no tiles.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.  The fp32 -> fp16 rounding is
// written out in ref_contract.h (h16), not taken from a library; tests/test_post_ref.py checks it against numpy over
// every case, through --h16, and against h2f over every half, through --roundtrip.
//
//   post_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, levels, tonemap, variant; float exposure, bloom_threshold,
//       bloom_intensity; uint16 color[H][W][4] (fp16 bit patterns).
// <out>: uint16 color[H][W][4] after the pass; then per level i < levels: uint32 w_i, h_i, uint16 B_i[h_i][w_i][4],
//        uint16 U_i[h_i][w_i][4].
//   post_ref --h16 <in> <out>: <in> is floats, <out> their h16 bit patterns.
//   post_ref --roundtrip <in> <out>: <in> is fp16 bit patterns, <out> each one's h16(h2f()).
// variant 0 is the contract.  1 .. 6 are deliberately wrong (the tests check that each one is told apart):
//   1 the blur's upper edge clamp is off by one     2 the box taps sit on 2x-1, 2x     3 the upsample weights are swapped
//   4 the threshold is applied before the box       5 the input's san is missing       6 the blur runs vertical first
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

struct Img {  // three fp32 channels
  uint32_t w = 0, h = 0;
  std::vector<float> v;
  Img() {}
  Img(uint32_t w_, uint32_t h_) : w(w_), h(h_), v((size_t)w_ * h_ * 3, 0.0f) {}
  float& at(uint32_t x, uint32_t y, int c) { return v[((size_t)y * w + x) * 3 + c]; }
  float at(uint32_t x, uint32_t y, int c) const { return v[((size_t)y * w + x) * 3 + c]; }
};

// C23
Img box(const Img& S) {
  Img D((S.w + 1) / 2, (S.h + 1) / 2);
  for (uint32_t y = 0; y < D.h; y++)
    for (uint32_t x = 0; x < D.w; x++) {
      uint32_t x0 = 2 * x, x1 = 2 * x + 1 < S.w - 1 ? 2 * x + 1 : S.w - 1;
      uint32_t y0 = 2 * y, y1 = 2 * y + 1 < S.h - 1 ? 2 * y + 1 : S.h - 1;
      if (g_variant == 2) {
        x0 = clampi(2 * (int64_t)x - 1, S.w), x1 = clampi(2 * (int64_t)x, S.w);
        y0 = clampi(2 * (int64_t)y - 1, S.h), y1 = clampi(2 * (int64_t)y, S.h);
      }
      for (int c = 0; c < 3; c++) D.at(x, y, c) = ((S.at(x0, y0, c) + S.at(x1, y0, c)) + (S.at(x0, y1, c) + S.at(x1, y1, c))) * 0.25f;
    }
  return D;
}

// C24: one direction of the blur
Img blur1(const Img& S, bool horizontal) {
  static const float wgt[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
  Img R(S.w, S.h);
  const uint32_t n = horizontal ? S.w : S.h;
  const uint32_t top = g_variant == 1 && n > 1 ? n - 1 : n;  // variant 1: the last texel is never a tap
  for (uint32_t y = 0; y < S.h; y++)
    for (uint32_t x = 0; x < S.w; x++)
      for (int c = 0; c < 3; c++) {
        float acc = 0.0f;
        for (int k = 0; k < 5; k++) {
          const uint32_t p = clampi((int64_t)(horizontal ? x : y) + k - 2, top);
          const float t = horizontal ? S.at(p, y, c) : S.at(x, p, c);
          acc = k == 0 ? t * wgt[0] : std::fma(t, wgt[k], acc);
        }
        R.at(x, y, c) = acc;
      }
  return R;
}

Img round16(const Img& S) {
  Img R = S;
  for (float& f : R.v) f = h2f(h16(f));
  return R;
}

// C25: one texel of up(S) at (x, y)
float up(const Img& S, uint32_t x, uint32_t y, int c) {
  const float fx = (float)x * 0.5f - 0.25f, fy = (float)y * 0.5f - 0.25f;
  const float flx = std::floor(fx), fly = std::floor(fy);
  float tx = fx - flx, ty = fy - fly;
  if (g_variant == 3) tx = 1.0f - tx, ty = 1.0f - ty;
  const uint32_t x0 = clampi((int64_t)flx, S.w), x1 = clampi((int64_t)flx + 1, S.w);
  const uint32_t y0 = clampi((int64_t)fly, S.h), y1 = clampi((int64_t)fly + 1, S.h);
  const float topv = std::fma(tx, S.at(x1, y0, c) - S.at(x0, y0, c), S.at(x0, y0, c));
  const float botv = std::fma(tx, S.at(x1, y1, c) - S.at(x0, y1, c), S.at(x0, y1, c));
  return std::fma(ty, botv - topv, topv);
}

void put_level(FILE* f, const Img& L) {
  std::vector<uint16_t> o((size_t)L.w * L.h * 4, 0);
  for (size_t i = 0; i < (size_t)L.w * L.h; i++)
    for (int c = 0; c < 3; c++) o[i * 4 + c] = h16(L.v[i * 3 + c]);
  std::fwrite(o.data(), 2, o.size(), f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "--h16") == 0) {
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<float> in;
    float buf[4096];
    size_t n;
    while ((n = std::fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    std::vector<uint16_t> out(in.size());
    for (size_t i = 0; i < in.size(); i++) out[i] = h16(in[i]);
    f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 2, out.size(), f);
    return std::fclose(f) == 0 ? 0 : 4;
  }
  if (argc == 4 && std::strcmp(argv[1], "--roundtrip") == 0) {
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint16_t> v;
    uint16_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 2, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    for (uint16_t& h : v) h = h16(h2f(h));
    f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(v.data(), 2, v.size(), f);
    return std::fclose(f) == 0 ? 0 : 4;
  }
  if (argc != 3) {
    std::fprintf(stderr, "usage: post_ref <in> <out> | post_ref --h16 <in> <out> | post_ref --roundtrip <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[9];
  float par[3];
  if (std::fread(hdr, 4, 9, f) != 9 || std::fread(par, 4, 3, f) != 3) return 3;
  const uint32_t W = hdr[0], H = hdr[1], sx = hdr[2], sy = hdr[3], sw = hdr[4], sh = hdr[5], levels = hdr[6], tonemap = hdr[7];
  g_variant = (int)hdr[8];
  const float exposure = par[0], threshold = par[1], intensity = par[2];
  if (sw == 0 || sh == 0 || sx + sw > W || sy + sh > H || levels > 8 || tonemap > 2) return 3;
  std::vector<uint16_t> color((size_t)W * H * 4);
  if (std::fread(color.data(), 2, color.size(), f) != color.size()) return 3;
  std::fclose(f);

  // the scissor is the image
  Img I(sw, sh);
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++)
      for (int c = 0; c < 3; c++) I.at(x, y, c) = h2f(color[((size_t)(sy + y) * W + sx + x) * 4 + c]);

  // C23, C24: the levels
  std::vector<Img> B(levels), U(levels);
  for (uint32_t i = 0; i < levels; i++) {
    Img D;
    if (i == 0) {
      Img S = I;
      if (g_variant == 4) {
        for (float& v : S.v) v = san(san(v) * exposure - threshold);
        D = box(S);
      } else {
        if (g_variant != 5)
          for (float& v : S.v) v = san(v);
        D = box(S);
        for (float& v : D.v) v = san(v * exposure - threshold);
      }
    } else {
      D = box(B[i - 1]);
    }
    B[i] = round16(g_variant == 6 ? blur1(blur1(D, false), true) : blur1(blur1(D, true), false));
  }
  // C25
  for (int i = (int)levels - 1; i >= 0; i--) {
    if (i == (int)levels - 1) {
      U[i] = B[i];
      continue;
    }
    U[i] = Img(B[i].w, B[i].h);
    for (uint32_t y = 0; y < B[i].h; y++)
      for (uint32_t x = 0; x < B[i].w; x++)
        for (int c = 0; c < 3; c++) {
          const float s = B[i].at(x, y, c) + up(U[i + 1], x, y, c);
          U[i].at(x, y, c) = h2f(h16(s < 65504.0f ? s : 65504.0f));
        }
  }
  // C26
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++)
      for (int c = 0; c < 3; c++) {
        const float bloom = levels >= 1 ? up(U[0], x, y, c) : 0.0f;
        const float h = san(std::fma(intensity, bloom, exposure * I.at(x, y, c)));
        float o;
        if (tonemap == 0) {
          o = h < 1.0f ? h : 1.0f;
        } else if (tonemap == 1) {
          o = h / (1.0f + h);
        } else {
          const float n = h * std::fma(2.51f, h, 0.03f);
          const float d = std::fma(h, std::fma(2.43f, h, 0.59f), 0.14f);
          o = n / d;
          o = o < 1.0f ? o : 1.0f;
        }
        color[((size_t)(sy + y) * W + sx + x) * 4 + c] = h16(o);
      }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(color.data(), 2, color.size(), f);
  for (uint32_t i = 0; i < levels; i++) {
    const uint32_t ext[2] = {B[i].w, B[i].h};
    std::fwrite(ext, 4, 2, f);
    put_level(f, B[i]);
    put_level(f, U[i]);
  }
  return std::fclose(f) == 0 ? 0 : 4;
}
