// exposure_ref — scalar restatement of auto-exposure's contract (include/svr_exposure.h) for the
// tests: one pixel at a time, one bin at a time.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE operation and std::fma the only fused one.  C41's 2^x is ref_contract.h's
// exp2_poly.
//
//   exposure_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, snap, variant; float key, low_fraction, high_fraction, min_exposure,
//       max_exposure, adapt; the previous state (float exposure, target, mean_log2; uint32 counted, black, meters);
//       uint16 color[H][W][4] (fp16 bit patterns).
// <out>: uint32 histogram[256]; the new state.
//   exposure_ref --exp2 <in> <out>: <in> is floats x, <out> the contract's 2^x as floats.
//   exposure_ref --bin <in> <out>:  <in> is luminances (floats), <out> their counters as uint32 (256: black).
// variant 0 is the contract.  1 .. 7 are deliberately wrong (the tests check that each one is told apart):
//   1 the bin shift is 19 (sixteen bins per octave)   2 black pixels are counted in bin 0
//   3 the window is taken over all pixels, black included   4 floor where the window's upper end says ceil
//   5 the clamp is applied after the adapt step, not to the target   6 the snap is ignored
//   7 the sub-bin literals are those of the bins' lower edges
#include <vector>

#include "ref_contract.h"

namespace {

int g_variant = 0;

// C38
float luminance(float r, float g, float b) { return std::fma(0.0722f, san(b), std::fma(0.7152f, san(g), 0.2126f * san(r))); }

// C39: 0 .. 255, or 256 for black
uint32_t counter_of(float L) {
  if (L < 0x1p-16f) return g_variant == 2 ? 0u : 256u;
  uint32_t bin = g_variant == 1 ? (bits(L) >> 19) - 1776u : (bits(L) >> 20) - 888u;
  return bin < 255u ? bin : 255u;
}

// C40: log2(1 + (j + 1/2) / 8)
const double kSubLog2[8] = {0x1.663f6fac91316p-4, 0x1.fbc16b902680ap-3, 0x1.91bba891f1709p-2, 0x1.0c10500d63aa6p-1,
                            0x1.49a784bcd1b8bp-1, 0x1.82809d5be7073p-1, 0x1.b74948f5532dap-1, 0x1.e88c6b3626a73p-1};

struct Meter {
  float key, low, high, min_exposure, max_exposure, adapt;
};
struct State {
  float exposure, target, mean_log2;
  uint32_t counted, black, meters;
};

int slurp(const char* path, std::vector<float>& out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  float buf[4096];
  size_t n;
  while ((n = std::fread(buf, 4, 4096, f)) > 0) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && (std::strcmp(argv[1], "--exp2") == 0 || std::strcmp(argv[1], "--bin") == 0)) {
    std::vector<float> in;
    if (int e = slurp(argv[2], in)) return e;
    std::vector<uint32_t> out(in.size());
    const bool e2 = argv[1][2] == 'e';
    for (size_t i = 0; i < in.size(); i++) out[i] = e2 ? bits(exp2_poly(in[i])) : counter_of(in[i]);
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    return std::fclose(f) == 0 ? 0 : 4;
  }
  if (argc != 3) {
    std::fprintf(stderr, "usage: exposure_ref <in> <out> | exposure_ref --exp2 <in> <out> | exposure_ref --bin <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[8];
  Meter m;
  State st;
  static_assert(sizeof(Meter) == 24 && sizeof(State) == 24, "layout");
  if (std::fread(hdr, 4, 8, f) != 8 || std::fread(&m, 24, 1, f) != 1 || std::fread(&st, 24, 1, f) != 1) return 3;
  const uint32_t W = hdr[0], H = hdr[1], sx = hdr[2], sy = hdr[3], sw = hdr[4], sh = hdr[5];
  const bool snap = hdr[6] != 0;
  g_variant = (int)hdr[7];
  if (sx + sw > W || sy + sh > H) return 3;
  std::vector<uint16_t> color((size_t)W * H * 4);
  if (std::fread(color.data(), 2, color.size(), f) != color.size()) return 3;
  std::fclose(f);

  uint32_t hist[257] = {0};
  for (uint32_t y = 0; y < sh; y++)
    for (uint32_t x = 0; x < sw; x++) {
      const uint16_t* t = &color[((size_t)(sy + y) * W + sx + x) * 4];
      hist[counter_of(luminance(h2f(t[0]), h2f(t[1]), h2f(t[2])))]++;
    }

  // C40
  uint32_t T = 0;
  for (int i = 0; i < 256; i++) T += hist[i];
  const uint32_t ranked = g_variant == 3 ? T + hist[256] : T;  // variant 3: ranks run over the black pixels too, which sort first
  const uint32_t lo = (uint32_t)std::floor((double)m.low * (double)ranked);
  const uint32_t hi = g_variant == 4 ? (uint32_t)std::floor((double)m.high * (double)ranked) : (uint32_t)std::ceil((double)m.high * (double)ranked);
  uint32_t kept = 0, sub[8] = {0};
  uint64_t octaves = 0;
  uint32_t begin = g_variant == 3 ? hist[256] : 0u;
  for (uint32_t i = 0; i < 256; i++) {
    const uint32_t end = begin + hist[i];
    const uint32_t from = begin > lo ? begin : lo, to = end < hi ? end : hi;
    const uint32_t k = to > from ? to - from : 0u;
    kept += k;
    octaves += (uint64_t)(i >> 3) * k;
    sub[i & 7u] += k;
    begin = end;
  }
  st.counted = T;
  st.black = hist[256];
  st.meters += 1u;
  if (kept != 0u) {
    double acc = (double)((int64_t)octaves - 16 * (int64_t)kept);
    for (int j = 0; j < 8; j++) acc = acc + (double)sub[j] * (g_variant == 7 ? std::log2(1.0 + j / 8.0) : kSubLog2[j]);
    const float mean_log2 = (float)(acc / (double)kept);
    // C42
    const float raw = m.key * exp2_poly(-mean_log2);
    float target = raw < m.min_exposure ? m.min_exposure : (raw > m.max_exposure ? m.max_exposure : raw);
    if (g_variant == 5) target = raw;
    st.mean_log2 = mean_log2;
    float e = (snap && g_variant != 6) ? target : std::fma(m.adapt, target - st.exposure, st.exposure);
    if (g_variant == 5) e = e < m.min_exposure ? m.min_exposure : (e > m.max_exposure ? m.max_exposure : e);
    st.target = target;
    st.exposure = e;
  }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(hist, 4, 256, f);
  std::fwrite(&st, 24, 1, f);
  return std::fclose(f) == 0 ? 0 : 4;
}
