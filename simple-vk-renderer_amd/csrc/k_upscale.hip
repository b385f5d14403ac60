// k_upscale.hip — the upscaled present (include/svr_upscale.h): the colour target magnified to the swapchain extent with a
// Catmull-Rom filter and an anti-ringing clamp, then sharpened at output resolution, in one kernel.  Arithmetic: DESIGN.md
// C50-C54; the bounds, the LDS budget and the bank behaviour: DESIGN.md §5 "Upscaled present".
//
//   upscale_kernel<FMT, SHARPEN>   one workgroup of 256 lanes per 32 x 16 tile of the destination, in five steps with a
//                                  barrier between them:
//     tables    per axis, for the tile's 34 output columns / 18 rows (the tile and the sharpen's one-pixel halo, output
//               indices clamped to the image): the four weights and the first tap's index in the staged window
//     stage     the 38 x 22 source texels the tile reaches, fetched at clamped coordinates, decoded, saturated and kept in
//               LDS as fp32, the four channels of a texel side by side (one 16-byte LDS access per tap): the arrays hold
//               the edge-clamped image and no tap needs a test
//     rows      the horizontal filter of every staged row at the 34 columns, into a second LDS array
//     columns   the vertical filter and the anti-ringing clamp at the 34 x 18 positions, into a third
//     finish    a lane per pixel: the sharpen out of LDS (or nothing, without it), un8, the texel packed in the
//               destination's channel order into an LDS tile (over the second array, which is dead by then); then a lane
//               per four pixels of a row: one 16-byte store where the piece is aligned and inside, else a texel at a time
// Every LDS index is a clamped integer out of the tables or a loop counter below an array's extent.  Ordinary vector loads
// and stores only; nothing is handed between workgroups.  The kernel reads the context's poison flag first: after an
// overflow it writes nothing but the present's status word, as blit_kernel does.
#include "svr_launch.h"
#include "svr_pixel.h"

namespace svr {

namespace {

constexpr uint32_t UT = 32, UTY = 16;          // the tile of the destination a workgroup writes: 32 wide, 16 high
constexpr uint32_t UP = UT + 2, UPY = UTY + 2;  // ... with the sharpen's halo
// the staged source texels per side: n outputs at a scale <= 1 reach at most n + 4
constexpr uint32_t US = UP + 4, USY = UPY + 4;

__device__ __forceinline__ float sat(float v) { return v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; }  // C50
__device__ __forceinline__ float lo2(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float hi2(float a, float b) { return a > b ? a : b; }

// C51: the first of the two central taps of output index i, and the fraction
__device__ __forceinline__ int tap0(uint32_t i, float scale, float& t) {
  const float u = ((float)i + 0.5f) * scale - 0.5f;
  const float f = floorf(u);
  t = u - f;
  return (int)f;
}

// C52: the filter of four taps
__device__ __forceinline__ float filter4(float w0, float w1, float w2, float w3, float s0, float s1, float s2, float s3) {
  return fmaf(w3, s3, fmaf(w2, s2, fmaf(w1, s1, w0 * s0)));
}

// C53 for one channel; `/` is correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
__device__ __forceinline__ float sharpen(float m, float n, float s, float e, float w, float peak) {
  const float lo = lo2(lo2(lo2(n, s), lo2(e, w)), m), hi = hi2(hi2(hi2(n, s), hi2(e, w)), m);
  const float a = hi > 0.0f ? lo2(lo, 1.0f - hi) / hi : 0.0f;
  const float k = a * peak;
  return fmaf(k, (n + s) + (e + w), m) / fmaf(4.0f, k, 1.0f);
}

// the four channels of a texel travel together: one 16-byte LDS access per tap
__device__ __forceinline__ float4 filter4(float4 w, float4 s0, float4 s1, float4 s2, float4 s3) {
  return make_float4(filter4(w.x, w.y, w.z, w.w, s0.x, s1.x, s2.x, s3.x), filter4(w.x, w.y, w.z, w.w, s0.y, s1.y, s2.y, s3.y),
                     filter4(w.x, w.y, w.z, w.w, s0.z, s1.z, s2.z, s3.z), filter4(w.x, w.y, w.z, w.w, s0.w, s1.w, s2.w, s3.w));
}
// C52's clamp into the range of the four central texels
__device__ __forceinline__ float ring(float p, float c00, float c10, float c01, float c11) {
  const float lo = lo2(lo2(c00, c10), lo2(c01, c11)), hi = hi2(hi2(c00, c10), hi2(c01, c11));
  return lo2(hi2(p, lo), hi);
}

}  // namespace

template <int FMT, bool SHARPEN>
__global__ __launch_bounds__(256) void upscale_kernel(UpscaleLaunch A, uint32_t status_ok) {
  const uint32_t void_op = *A.poison;
  if (A.status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *A.status = void_op ? 1u : status_ok;
  if (void_op) return;
  __shared__ float4 s_src[USY][US];  // s at clamped coordinates
  __shared__ float4 s_h[USY][UP];   // its rows filtered; later the packed texels of the tile
  __shared__ float4 s_p[UPY][UP];   // P
  __shared__ float4 s_w[2][UP];     // per axis: the four weights of each output column / row
  __shared__ int s_l[2][UP];        // ... and its first tap's index in the window, 0 .. US - 4 (columns), 0 .. USY - 4 (rows)
  const uint32_t t = threadIdx.x;
  const uint32_t tx0 = blockIdx.x * UT, ty0 = blockIdx.y * UTY;
  // the window's origin: the first tap of the tile's first output (with halo), per axis
  float frac;
  const int ox = tap0(clamp_to((int)tx0 - 1, A.dw), A.su, frac) - 1;
  const int oy = tap0(clamp_to((int)ty0 - 1, A.dh), A.sv, frac) - 1;

  if (t < 128u && (t & 63u) < (t < 64u ? UP : UPY)) {  // lanes 0..33 of the first wave: columns; 0..17 of the second: rows
    const uint32_t axis = t >> 6, k = t & 63u;
    const uint32_t i = clamp_to((int)((axis ? ty0 : tx0) + k) - 1, axis ? A.dh : A.dw);
    const int first = tap0(i, axis ? A.sv : A.su, frac) - 1 - (axis ? oy : ox);
    s_l[axis][k] = min(max(first, 0), (int)((axis ? USY : US) - 4u));  // (never binds: DESIGN.md §5; no input can index outside the window)
    const float f = frac;
    s_w[axis][k] = make_float4(fmaf(fmaf(-0.5f, f, 1.0f), f, -0.5f) * f, fmaf(fmaf(1.5f, f, -2.5f), f * f, 1.0f),
                               fmaf(fmaf(-1.5f, f, 2.0f), f, 0.5f) * f, fmaf(0.5f, f, -0.5f) * (f * f));
  }

  typedef typename Codec<FMT>::enc_t enc_t;
  const enc_t* src = reinterpret_cast<const enc_t*>(A.src);
  for (uint32_t i = t; i < USY * US; i += 256u) {
    const uint32_t r = i / US, c = i - r * US;
    const uint32_t x = clamp_to(ox + (int)c, A.W), y = clamp_to(oy + (int)r, A.H);
    const float4 v = Codec<FMT>::decode(src[(size_t)y * A.W + x]);
    s_src[r][c] = make_float4(sat(v.x), sat(v.y), sat(v.z), sat(v.w));
  }
  __syncthreads();

  for (uint32_t i = t; i < USY * UP; i += 256u) {
    const uint32_t r = i / UP, c = i - r * UP;
    const float4* p = &s_src[r][s_l[0][c]];
    s_h[r][c] = filter4(s_w[0][c], p[0], p[1], p[2], p[3]);
  }
  __syncthreads();

  for (uint32_t i = t; i < UPY * UP; i += 256u) {
    const uint32_t r = i / UP, c = i - r * UP;
    if (!SHARPEN && (r == 0u || r == UPY - 1u || c == 0u || c == UP - 1u)) continue;  // the halo feeds the sharpen only
    const int lx = s_l[0][c], ly = s_l[1][r];
    const float4 p = filter4(s_w[1][r], s_h[ly][c], s_h[ly + 1][c], s_h[ly + 2][c], s_h[ly + 3][c]);
    const float4 c00 = s_src[ly + 1][lx + 1], c10 = s_src[ly + 1][lx + 2], c01 = s_src[ly + 2][lx + 1], c11 = s_src[ly + 2][lx + 2];
    s_p[r][c] = make_float4(ring(p.x, c00.x, c10.x, c01.x, c11.x), ring(p.y, c00.y, c10.y, c01.y, c11.y), ring(p.z, c00.z, c10.z, c01.z, c11.z),
                            ring(p.w, c00.w, c10.w, c01.w, c11.w));
  }
  __syncthreads();

  uint32_t* s_out = reinterpret_cast<uint32_t*>(&s_h[0][0]);  // UT x UTY texels: s_h was last read before the barrier above
  {
    const uint32_t c = t % UT;
#pragma unroll
    for (uint32_t j = 0; j < UTY / 8u; j++) {
      const uint32_t r = t / UT + 8u * j;
      float4 o = s_p[r + 1u][c + 1u];
      if (SHARPEN) {
        const float4 n = s_p[r][c + 1u], so = s_p[r + 2u][c + 1u], e = s_p[r + 1u][c + 2u], w = s_p[r + 1u][c];
        o = make_float4(sharpen(o.x, n.x, so.x, e.x, w.x, A.peak), sharpen(o.y, n.y, so.y, e.y, w.y, A.peak), sharpen(o.z, n.z, so.z, e.z, w.z, A.peak), o.w);
      }
      const uint32_t red = un8(o.x), green = un8(o.y), blue = un8(o.z), alpha = un8(o.w);
      s_out[r * UT + c] = A.dst_fmt == SVR_SWAPCHAIN_B8G8R8A8 ? (blue | (green << 8) | (red << 16) | (alpha << 24))
                                                              : (red | (green << 8) | (blue << 16) | (alpha << 24));
    }
  }
  __syncthreads();

  const uint32_t row = t / 8u, piece = (t % 8u) * 4u, x = tx0 + piece, y = ty0 + row;
  if (row >= UTY || x >= A.dw || y >= A.dh) return;
  const uint4 q = *reinterpret_cast<const uint4*>(s_out + row * UT + piece);
  uint32_t* at = A.dst + (size_t)y * A.dw + x;
  if (x + 3u < A.dw && aligned_to(at, 16u)) {
    *reinterpret_cast<uint4*>(at) = q;
  } else {
    at[0] = q.x;
    if (x + 1u < A.dw) at[1] = q.y;
    if (x + 2u < A.dw) at[2] = q.z;
    if (x + 3u < A.dw) at[3] = q.w;
  }
}

void launch_upscale(const UpscaleLaunch& A, uint32_t status_ok, hipStream_t s) {
  const dim3 grid((A.dw + UT - 1u) / UT, (A.dh + UTY - 1u) / UTY), block(256);
  if (A.src_fmt == SVR_COLOR_RGBA16F) {
    if (A.sharpen) hipLaunchKernelGGL((upscale_kernel<SVR_COLOR_RGBA16F, true>), grid, block, 0, s, A, status_ok);
    else hipLaunchKernelGGL((upscale_kernel<SVR_COLOR_RGBA16F, false>), grid, block, 0, s, A, status_ok);
  } else {
    if (A.sharpen) hipLaunchKernelGGL((upscale_kernel<SVR_COLOR_RGBA8, true>), grid, block, 0, s, A, status_ok);
    else hipLaunchKernelGGL((upscale_kernel<SVR_COLOR_RGBA8, false>), grid, block, 0, s, A, status_ok);
  }
}

}  // namespace svr
