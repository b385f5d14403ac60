// The texel arena's tiled mip layout (csrc/svr_device.h: mip_offset, level_lw/level_lh/level_bytes, texel_offset), on the
// host: for every extent pair the address function must map each level one-to-one into that level's own padded span,
// consecutive spans must not overlap, and mip_offset must be the running sum of the padded level sizes.
// Prints "levels N texels M ok", or the first violation and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#include "texel_layout_under_test.h"

using namespace svr_layout;

static int check(uint32_t w, uint32_t h, unsigned long long* n_levels, unsigned long long* n_texels) {
  uint32_t lw = 0, lh = 0, levels = 1;
  while ((1u << lw) < w) lw++;
  while ((1u << lh) < h) lh++;
  for (uint32_t m = std::max(w, h); m > 1; m >>= 1) levels++;
  uint64_t sum = 0;  // of the padded sizes of the levels before this one
  std::vector<uint8_t> seen;
  for (uint32_t l = 0; l < levels; l++) {
    const uint32_t wl = std::max(w >> l, 1u), hl = std::max(h >> l, 1u);
    const uint32_t plw = level_lw(lw, l), plh = level_lh(lh, l), bytes = level_bytes(lw, lh, l);
    if (mip_offset(lw, lh, l) != sum) return std::printf("%ux%u level %u: mip_offset %u, levels before it hold %llu\n", w, h, l, mip_offset(lw, lh, l), (unsigned long long)sum), 1;
    if (bytes != (4u << (plw + plh)) || bytes % TEX_TILE_BYTES || wl > (1u << plw) || hl > (1u << plh))
      return std::printf("%ux%u level %u: padded extent 2^%u x 2^%u, %u bytes\n", w, h, l, plw, plh, bytes), 1;
    seen.assign(bytes / 4, 0);
    for (uint32_t y = 0; y < hl; y++)
      for (uint32_t x = 0; x < wl; x++) {
        const uint32_t o = texel_offset(plw, x, y);
        if (o != texel_offset_x(x) + texel_offset_y(plw, y)) return std::printf("%ux%u level %u (%u,%u): parts do not add up\n", w, h, l, x, y), 1;
        if ((o & 3u) || o >= bytes) return std::printf("%ux%u level %u (%u,%u): offset %u outside the level's %u bytes\n", w, h, l, x, y, o, bytes), 1;
        if (seen[o / 4]++) return std::printf("%ux%u level %u (%u,%u): offset %u taken twice\n", w, h, l, x, y, o), 1;
        // a tile is one aligned block: texels of the same tile share it, others do not
        const uint32_t tile = (y >> TEX_TILE_LH) * (1u << (plw - TEX_TILE_LW)) + (x >> TEX_TILE_LW);
        if (o / TEX_TILE_BYTES != tile) return std::printf("%ux%u level %u (%u,%u): block %u, tile %u\n", w, h, l, x, y, o / TEX_TILE_BYTES, tile), 1;
        ++*n_texels;
      }
    sum += bytes;
    ++*n_levels;
  }
  return 0;
}

int main() {
  unsigned long long n_levels = 0, n_texels = 0;
  for (uint32_t h = 1; h <= 40; h++)
    for (uint32_t w = 1; w <= 40; w++)
      if (check(w, h, &n_levels, &n_texels)) return 1;
  const uint32_t extra[][2] = {{1024, 4}, {4, 1024}, {16384, 1}, {1, 16384}, {1024, 1024}};
  for (const auto& e : extra)
    if (check(e[0], e[1], &n_levels, &n_texels)) return 1;
  std::printf("levels %llu texels %llu ok\n", n_levels, n_texels);
  return 0;
}
