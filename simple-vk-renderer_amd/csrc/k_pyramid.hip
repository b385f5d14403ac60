// k_pyramid.hip — the min-depth pyramid of occlusion culling (include/svr_occlusion.h).
//
// Texel (x, y) of level l is the minimum, over the uint32 bit patterns, of the depth pixels of [x 2^l, (x + 1) 2^l) x
// [y 2^l, (y + 1) 2^l) inside the frame.  One launch reduces a level s into the next PYR_STEP levels: a workgroup takes
// a 64 x 64 block of level s (aligned, so each of its texels of level s + j covers whole 2^j x 2^j groups of the block),
// reads it once — coalesced rows, 16 bytes per lane where the rows are 16-byte aligned — and halves it through LDS six
// times.  Texels outside level s read as the identity 0xffffffff, so partial blocks at the frame's right and bottom edges
// need no rule of their own; texels outside a level's extent are not stored.  The levels past the first six come from
// further launches over level 6, 12: a kernel boundary between them, no hand-off between workgroups inside a launch.
// Ordinary vector stores only.  Every launch reads the context's poison flag first: after an overflow it writes nothing.
#include <algorithm>

#include "svr_launch.h"

namespace svr {

constexpr uint32_t PYR_STEP = 6;  // levels one launch makes: 64 -> 1 texel per block side

struct PyrLaunch {
  const uint32_t* src;          // level s (the depth target when s = 0), sw x sh, row-major
  uint32_t sw, sh;
  uint32_t vec;                 // 1: rows of src are 16-byte aligned (uint4 loads)
  uint32_t n_out;               // levels s + 1 .. s + n_out
  uint32_t* dst[PYR_STEP];
  uint32_t dw[PYR_STEP], dh[PYR_STEP];
  const uint32_t* poison;
};

__global__ __launch_bounds__(256) void pyramid_kernel(PyrLaunch L) {
  if (*L.poison) return;
  __shared__ uint32_t s_a[32 * 32], s_b[16 * 16];
  const uint32_t t = threadIdx.x, x0 = blockIdx.x * 64u, y0 = blockIdx.y * 64u;
  // level s + 1: four rounds of 16 rows; lane t reads 4 texels of row 16 i + t / 16 and folds them with the 4 of the
  // row next to it (lane t ^ 16, same wave)
  const uint32_t cx = x0 + 4u * (t & 15u);
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t r = 16u * i + (t >> 4), y = y0 + r;
    uint32_t v[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (y < L.sh) {
      const uint32_t* row = L.src + (size_t)y * L.sw;
      if (L.vec && cx + 3u < L.sw) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + cx);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
          if (cx + k < L.sw) v[k] = row[cx + k];
      }
    }
    uint32_t h0 = min(v[0], v[1]), h1 = min(v[2], v[3]);
    h0 = min(h0, (uint32_t)__shfl_xor((int)h0, 16));
    h1 = min(h1, (uint32_t)__shfl_xor((int)h1, 16));
    if (((t >> 4) & 1u) == 0u) {
      const uint32_t lx = 2u * (t & 15u), ly = r >> 1;
      s_a[ly * 32u + lx] = h0;
      s_a[ly * 32u + lx + 1u] = h1;
      const uint32_t gx = x0 / 2u + lx, gy = y0 / 2u + ly;
      if (gy < L.dh[0]) {
        uint32_t* out = L.dst[0] + (size_t)gy * L.dw[0] + gx;  // (gx is even)
        if (gx + 1u < L.dw[0] && (reinterpret_cast<uintptr_t>(out) & 7u) == 0u) {
          *reinterpret_cast<uint2*>(out) = make_uint2(h0, h1);  // one 8-byte store where the pair is aligned
        } else {
          if (gx < L.dw[0]) out[0] = h0;
          if (gx + 1u < L.dw[0]) out[1] = h1;
        }
      }
    }
  }
  // levels s + 2 .. s + n_out: n x n texels of the block in `cur` -> n/2 x n/2 in `nxt`
  uint32_t* cur = s_a;
  uint32_t* nxt = s_b;
  uint32_t n = 32u;
  for (uint32_t k = 1; k < L.n_out; k++) {
    __syncthreads();
    const uint32_t m = n >> 1;
    if (t < m * m) {
      const uint32_t tx = t % m, ty = t / m;
      const uint32_t* p = cur + 2u * ty * n + 2u * tx;
      const uint32_t v = min(min(p[0], p[1]), min(p[n], p[n + 1u]));
      nxt[t] = v;
      const uint32_t gx = blockIdx.x * m + tx, gy = blockIdx.y * m + ty;
      if (gx < L.dw[k] && gy < L.dh[k]) L.dst[k][(size_t)gy * L.dw[k] + gx] = v;
    }
    uint32_t* sw = cur;
    cur = nxt;
    nxt = sw;
    n = m;
  }
}

uint32_t pyramid_levels(uint32_t W, uint32_t H) {
  uint32_t l = 1;
  while (((W - 1u) >> l) != 0u || ((H - 1u) >> l) != 0u) l++;  // ceil(W / 2^l) = ((W - 1) >> l) + 1
  return l;
}

size_t pyramid_offsets(uint32_t W, uint32_t H, uint32_t* off) {
  const uint32_t n = pyramid_levels(W, H);
  size_t words = 0;
  off[0] = 0;
  for (uint32_t l = 1; l <= n; l++) {
    off[l] = (uint32_t)words;
    words += (size_t)(((W - 1u) >> l) + 1u) * (((H - 1u) >> l) + 1u);
  }
  return words;
}

void launch_pyramid(const float* depth, uint32_t W, uint32_t H, uint32_t* pyr, const uint32_t* off, uint32_t n_levels,
                    const uint32_t* poison, hipStream_t s) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(depth);
  uint32_t sw = W, sh = H;
  for (uint32_t l0 = 0; l0 < n_levels; l0 += PYR_STEP) {
    PyrLaunch L{};
    L.src = src;
    L.sw = sw;
    L.sh = sh;
    L.vec = (sw % 4u == 0u && reinterpret_cast<uintptr_t>(src) % 16u == 0u) ? 1u : 0u;
    L.n_out = std::min<uint32_t>(PYR_STEP, n_levels - l0);
    for (uint32_t k = 0; k < L.n_out; k++) {
      const uint32_t l = l0 + 1u + k;
      L.dst[k] = pyr + off[l];
      L.dw[k] = ((W - 1u) >> l) + 1u;
      L.dh[k] = ((H - 1u) >> l) + 1u;
    }
    L.poison = poison;
    hipLaunchKernelGGL(pyramid_kernel, dim3((sw + 63u) / 64u, (sh + 63u) / 64u), dim3(256), 0, s, L);
    src = L.dst[L.n_out - 1u];
    sw = L.dw[L.n_out - 1u];
    sh = L.dh[L.n_out - 1u];
  }
}

}  // namespace svr
