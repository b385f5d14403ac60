// light_ref — scalar, brute-force restatement of the lighting contract for the tests: every light is
// visited at every pixel, no tiles, no culling.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.  The chain of one pixel is
// ref_contract.h's light_pixel, which ambient_ref.cpp runs with the ambient factor.
//
//   light_ref <in> <out>
// <in>  (little endian): uint32 W, H, n_lights, Ws, Hs (Ws = Hs = 0: no shadow map); float inv_viewproj[16], ambient[4],
//       sun_direction[4], sun_color[4], shadow_viewproj[16], shadow_bias; n_lights x {float position[3], radius, color[3],
//       intensity}; float depth[H][W], normal[H][W][4], albedo[H][W][4], shadow[Hs][Ws].
// <out>: float rgba[H][W][4] (zeros where no winner); uint8 winner[H][W]; float position[H][W][3]; uint8 shadowed[H][W].
// The stores of C20 are the Python side's (numpy casts).
#include <vector>

#include "ref_contract.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: light_ref <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  LightFrame F;
  if (!read_all(f, &F, sizeof F)) return 3;
  const uint32_t W = F.W, H = F.H;
  const size_t n = (size_t)W * H;
  std::vector<Light> lights(F.n_lights);
  std::vector<float> depth(n), normal(n * 4), albedo(n * 4), shadow((size_t)F.Ws * F.Hs);
  if (!read_all(f, lights.data(), lights.size() * sizeof(Light)) || !read_all(f, depth.data(), n * 4) || !read_all(f, normal.data(), n * 16) ||
      !read_all(f, albedo.data(), n * 16) || !read_all(f, shadow.data(), shadow.size() * 4))
    return 3;
  std::fclose(f);

  std::vector<float> rgba(n * 4, 0.0f), position(n * 3, 0.0f);
  std::vector<uint8_t> winner(n, 0), in_shadow(n, 0);
  for (uint32_t py = 0; py < H; py++) {
    for (uint32_t px = 0; px < W; px++) {
      const size_t i = (size_t)py * W + px;
      if (bits(albedo[i * 4 + 3]) != 0x3F800000u) continue;
      winner[i] = 1;
      bool shadowed;
      light_pixel(F, lights.data(), shadow.data(), px, py, depth[i], &normal[i * 4], &albedo[i * 4], nullptr, &position[i * 3], shadowed, &rgba[i * 4]);
      in_shadow[i] = shadowed ? 1 : 0;
      rgba[i * 4 + 3] = 1.0f;
    }
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  bool ok = std::fwrite(rgba.data(), 4, rgba.size(), o) == rgba.size() && std::fwrite(winner.data(), 1, n, o) == n &&
            std::fwrite(position.data(), 4, position.size(), o) == position.size() && std::fwrite(in_shadow.data(), 1, n, o) == n;
  ok = std::fclose(o) == 0 && ok;
  return ok ? 0 : 4;
}
