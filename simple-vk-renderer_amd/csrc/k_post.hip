// k_post.hip — the HDR post pass (include/svr_post.h): exposure, bloom and a tone-mapping operator over the RGBA16F colour
// target, in place.  Arithmetic: DESIGN.md C22-C26; ordering and the replay argument: DESIGN.md §5 "Post pass".
//
// Three kernels, at most 2 L launches for L bloom levels (launch_post):
//   bloom_level_kernel<FIRST>   B_i from its source (the colour target's scissor for FIRST, else B_{i-1}).  One workgroup
//                               of 256 lanes per 32 x 32 tile of B_i: the 36 x 36 texels of D_i the tile's blur reaches
//                               are boxed from 2 x 2 source texels on the way into LDS (fp32, a plane per channel), the
//                               horizontal blur goes into a second LDS array (36 rows x 32), the vertical one into
//                               registers, and the tile is stored as 8-byte texels, 32 lanes to a row.
//   bloom_up_kernel             U_i in place over B_i: a lane reads its own texel and the four taps of U_{i+1}.
//   post_composite_kernel<OP>   two pixels (16 bytes in, 16 bytes out) per lane where the address allows, else one at a
//                               time; the taps of U_0 are re-reads of the half-resolution level, served by the caches.
// Under svr_set_post_auto_exposure (include/svr_exposure.h) the two kernels that use the exposure run as the instances
// that multiply it by the state's exposure, read through a pointer; the others' machine code is the parent's.
// Staged texels are fetched at clamped coordinates, so the LDS arrays hold the edge-clamped image and no tap needs a test.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch.  Every kernel reads the
// context's poison flag first: after an overflow it writes nothing.
#include "svr_launch.h"
#include "svr_pixel.h"

namespace svr {

namespace {

constexpr uint32_t PT = 32;       // the tile of a level image a workgroup writes
constexpr uint32_t PS = PT + 4;   // ... and the staged texels per side: two more each way for the five taps

// texels x0 and x1 (x1 == x0 + 1 or x1 == x0) of one row: one 16-byte load where the address allows
__device__ __forceinline__ void load_pair(const uint2* row, uint32_t x0, uint32_t x1, uint2& a, uint2& b) {
  if (x1 != x0 && aligned_to(row + x0, 16u)) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + x0);
    a = make_uint2(q.x, q.y);
    b = make_uint2(q.z, q.w);
  } else {
    a = row[x0];
    b = row[x1];
  }
}

// C25: up(S)(x, y), S a level image of ws x hs texels
__device__ __forceinline__ Rgb upsample(const uint2* S, uint32_t ws, uint32_t hs, uint32_t x, uint32_t y) {
  const float fx = (float)x * 0.5f - 0.25f, fy = (float)y * 0.5f - 0.25f;
  const float flx = floorf(fx), fly = floorf(fy);
  const float tx = fx - flx, ty = fy - fly;
  const uint32_t x0 = clamp_to((int)flx, ws), x1 = clamp_to((int)flx + 1, ws);
  const uint32_t y0 = clamp_to((int)fly, hs), y1 = clamp_to((int)fly + 1, hs);
  const uint2* r0 = S + (size_t)y0 * ws;
  const uint2* r1 = S + (size_t)y1 * ws;
  uint2 q00, q10, q01, q11;
  load_pair(r0, x0, x1, q00, q10);
  load_pair(r1, x0, x1, q01, q11);
  const Rgb a = decode_rgb(q00), b = decode_rgb(q10), c = decode_rgb(q01), d = decode_rgb(q11);
  const Rgb top = {fmaf(tx, b.r - a.r, a.r), fmaf(tx, b.g - a.g, a.g), fmaf(tx, b.b - a.b, a.b)};
  const Rgb bot = {fmaf(tx, d.r - c.r, c.r), fmaf(tx, d.g - c.g, c.g), fmaf(tx, d.b - c.b, c.b)};
  return {fmaf(ty, bot.r - top.r, top.r), fmaf(ty, bot.g - top.g, top.g), fmaf(ty, bot.b - top.b, top.b)};
}

}  // namespace

struct LevelArgs {
  const uint2* src;      // texel (0, 0) of the source image
  uint32_t src_pitch;    // texels per source row
  uint32_t ws, hs;       // the source's extent
  uint2* dst;            // B_i, w texels per row
  uint32_t w, h;
  float exposure, threshold;  // FIRST only
  const uint32_t* poison;
};

// C23 for one channel
template <bool FIRST>
__device__ __forceinline__ float box(float a00, float a10, float a01, float a11, float exposure, float threshold) {
  if (FIRST) {
    a00 = san(a00); a10 = san(a10); a01 = san(a01); a11 = san(a11);
  }
  const float v = ((a00 + a10) + (a01 + a11)) * 0.25f;
  return FIRST ? san(v * exposure - threshold) : v;
}

// State: nothing, or, under svr_set_post_auto_exposure, one `const float*` to the state's exposure (include/svr_exposure.h):
// e = pass.exposure * state.exposure then stands for the exposure.  The state is read behind the poison flag, like
// everything else.  (One kernel with its body in place: the instances without a state are the parent's machine code, which a
// body shared through an inlined function was not, by the operand order of four multiplies.)
template <bool FIRST, class... State>
__global__ __launch_bounds__(256) void bloom_level_kernel(LevelArgs A, State... state) {
  if (*A.poison) return;
  float exposure = A.exposure;
  if constexpr (sizeof...(State) != 0) exposure = exposure * *(state, ...);
  __shared__ float s_d[3][PS][PS];  // D_i at clamped coordinates
  __shared__ float s_h[3][PS][PT];  // its horizontal blur
  const uint32_t t = threadIdx.x;
  const uint32_t tx0 = blockIdx.x * PT, ty0 = blockIdx.y * PT;

  for (uint32_t i = t; i < PS * PS; i += 256u) {
    const uint32_t r = i / PS, c = i - r * PS;
    const uint32_t x = clamp_to((int)(tx0 + c) - 2, A.w), y = clamp_to((int)(ty0 + r) - 2, A.h);
    const uint32_t x0 = 2u * x, x1 = min(2u * x + 1u, A.ws - 1u), y0 = 2u * y, y1 = min(2u * y + 1u, A.hs - 1u);
    uint2 q00, q10, q01, q11;
    load_pair(A.src + (size_t)y0 * A.src_pitch, x0, x1, q00, q10);
    load_pair(A.src + (size_t)y1 * A.src_pitch, x0, x1, q01, q11);
    const Rgb a = decode_rgb(q00), b = decode_rgb(q10), cc = decode_rgb(q01), d = decode_rgb(q11);
    s_d[0][r][c] = box<FIRST>(a.r, b.r, cc.r, d.r, exposure, A.threshold);
    s_d[1][r][c] = box<FIRST>(a.g, b.g, cc.g, d.g, exposure, A.threshold);
    s_d[2][r][c] = box<FIRST>(a.b, b.b, cc.b, d.b, exposure, A.threshold);
  }
  __syncthreads();

  // C24: the weights are exact in fp32
  constexpr float W0 = 0.0625f, W1 = 0.25f, W2 = 0.375f;
  for (uint32_t i = t; i < PS * PT; i += 256u) {
    const uint32_t r = i / PT, c = i % PT;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float* p = &s_d[ch][r][c];
      float acc = p[0] * W0;
      acc = fmaf(p[1], W1, acc);
      acc = fmaf(p[2], W2, acc);
      acc = fmaf(p[3], W1, acc);
      acc = fmaf(p[4], W0, acc);
      s_h[ch][r][c] = acc;
    }
  }
  __syncthreads();

  const uint32_t c = t % PT, x = tx0 + c;
#pragma unroll
  for (uint32_t j = 0; j < 4u; j++) {
    const uint32_t r = t / PT + 8u * j, y = ty0 + r;
    float v[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      float acc = s_h[ch][r][c] * W0;
      acc = fmaf(s_h[ch][r + 1][c], W1, acc);
      acc = fmaf(s_h[ch][r + 2][c], W2, acc);
      acc = fmaf(s_h[ch][r + 3][c], W1, acc);
      acc = fmaf(s_h[ch][r + 4][c], W0, acc);
      v[ch] = acc;
    }
    if (x < A.w && y < A.h) A.dst[(size_t)y * A.w + x] = make_uint2(h16(v[0]) | (h16(v[1]) << 16), h16(v[2]));
  }
}

struct UpArgs {
  uint2* dst;        // B_i on entry, U_i on exit: w x h
  uint32_t w, h;
  const uint2* src;  // U_{i+1}: ws x hs
  uint32_t ws, hs;
  const uint32_t* poison;
};

__device__ __forceinline__ float add_clamped(float b, float u) {
  const float s = b + u;
  return s < HALF_MAX ? s : HALF_MAX;
}

__global__ __launch_bounds__(256) void bloom_up_kernel(UpArgs A) {
  if (*A.poison) return;
  const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (x >= A.w || y >= A.h) return;
  uint2* at = A.dst + (size_t)y * A.w + x;
  const Rgb b = decode_rgb(*at);
  const Rgb u = upsample(A.src, A.ws, A.hs, x, y);
  *at = make_uint2(h16(add_clamped(b.r, u.r)) | (h16(add_clamped(b.g, u.g)) << 16), h16(add_clamped(b.b, u.b)));
}

struct CompositeArgs {
  uint2* color;      // texel (0, 0) of the scissor
  uint32_t pitch;    // texels per row of the target
  uint32_t sw, sh;
  const uint2* u0;   // U_0: w0 x h0 (levels >= 1)
  uint32_t w0, h0;
  uint32_t levels;
  float exposure, intensity;
  const uint32_t* poison;
};

// C26 for one channel
template <int OP>
__device__ __forceinline__ float tonemap(float h) {
  if (OP == SVR_TONEMAP_CLAMP) return h < 1.0f ? h : 1.0f;
  // `/` is correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
  if (OP == SVR_TONEMAP_REINHARD) return h / (1.0f + h);
  const float n = h * fmaf(2.51f, h, 0.03f);
  const float d = fmaf(h, fmaf(2.43f, h, 0.59f), 0.14f);
  const float o = n / d;
  return o < 1.0f ? o : 1.0f;
}

template <int OP>
__device__ __forceinline__ uint2 composite_pixel(const CompositeArgs& A, uint2 texel, uint32_t x, uint32_t y) {
  Rgb bloom = {0.0f, 0.0f, 0.0f};
  if (A.levels) bloom = upsample(A.u0, A.w0, A.h0, x, y);
  const Rgb in = decode_rgb(texel);
  const float r = tonemap<OP>(san(fmaf(A.intensity, bloom.r, A.exposure * in.r)));
  const float g = tonemap<OP>(san(fmaf(A.intensity, bloom.g, A.exposure * in.g)));
  const float b = tonemap<OP>(san(fmaf(A.intensity, bloom.b, A.exposure * in.b)));
  return encode_rgb({r, g, b}, texel);
}

// the body of post_composite_kernel<OP> and of post_composite_auto_kernel<OP>
template <int OP>
__device__ __forceinline__ void post_composite(const CompositeArgs& A) {
  const uint32_t x = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 2u, y = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (x >= A.sw || y >= A.sh) return;
  uint2* at = A.color + (size_t)y * A.pitch + x;
  if (x + 1u < A.sw && aligned_to(at, 16u)) {
    const uint4 q = *reinterpret_cast<const uint4*>(at);
    const uint2 a = composite_pixel<OP>(A, make_uint2(q.x, q.y), x, y), b = composite_pixel<OP>(A, make_uint2(q.z, q.w), x + 1u, y);
    *reinterpret_cast<uint4*>(at) = make_uint4(a.x, a.y, b.x, b.y);
  } else {
    at[0] = composite_pixel<OP>(A, at[0], x, y);
    if (x + 1u < A.sw) at[1] = composite_pixel<OP>(A, at[1], x + 1u, y);
  }
}

template <int OP>
__global__ __launch_bounds__(256) void post_composite_kernel(CompositeArgs A) {
  if (*A.poison) return;
  post_composite<OP>(A);
}

// post_composite_kernel<OP> under svr_set_post_auto_exposure: e in the exposure's place, as in bloom_level_kernel<true, const float*>
template <int OP>
__global__ __launch_bounds__(256) void post_composite_auto_kernel(CompositeArgs A, const float* state_exposure) {
  if (*A.poison) return;
  A.exposure = A.exposure * *state_exposure;
  post_composite<OP>(A);
}

size_t post_level_layout(uint32_t sw, uint32_t sh, uint32_t n_levels, uint32_t* off, uint32_t* lw, uint32_t* lh) {
  size_t at = 0;
  uint32_t w = sw, h = sh;
  for (uint32_t i = 0; i < n_levels; i++) {
    w = (w + 1u) / 2u;
    h = (h + 1u) / 2u;
    off[i] = (uint32_t)at;
    lw[i] = w;
    lh[i] = h;
    at += ((size_t)w * h + 1u) & ~(size_t)1u;
  }
  return at;
}

void launch_post(const PostLaunch& P, hipStream_t s) {
  if (P.sw == 0u || P.sh == 0u) return;
  const dim3 block(256);
  uint2* scissor = P.color + (size_t)P.sy * P.W + P.sx;
  for (uint32_t i = 0; i < P.n_levels; i++) {
    LevelArgs A{};
    A.dst = P.levels + P.off[i];
    A.w = P.lw[i];
    A.h = P.lh[i];
    A.exposure = P.exposure;
    A.threshold = P.threshold;
    A.poison = P.poison;
    const dim3 grid((A.w + PT - 1u) / PT, (A.h + PT - 1u) / PT);
    if (i == 0u) {
      A.src = scissor;
      A.src_pitch = P.W;
      A.ws = P.sw;
      A.hs = P.sh;
      if (P.auto_exposure)
        hipLaunchKernelGGL(bloom_level_kernel<true>, grid, block, 0, s, A, P.auto_exposure);
      else
        hipLaunchKernelGGL(bloom_level_kernel<true>, grid, block, 0, s, A);
    } else {
      A.src = P.levels + P.off[i - 1u];
      A.src_pitch = A.ws = P.lw[i - 1u];
      A.hs = P.lh[i - 1u];
      hipLaunchKernelGGL(bloom_level_kernel<false>, grid, block, 0, s, A);
    }
  }
  for (uint32_t i = P.n_levels; i-- > 1u;) {  // U_{L-1} = B_{L-1}; U_i over B_i for i = L-2 .. 0
    UpArgs A{};
    A.dst = P.levels + P.off[i - 1u];
    A.w = P.lw[i - 1u];
    A.h = P.lh[i - 1u];
    A.src = P.levels + P.off[i];
    A.ws = P.lw[i];
    A.hs = P.lh[i];
    A.poison = P.poison;
    hipLaunchKernelGGL(bloom_up_kernel, dim3((A.w + 63u) / 64u, (A.h + 3u) / 4u), block, 0, s, A);
  }
  CompositeArgs C{};
  C.color = scissor;
  C.pitch = P.W;
  C.sw = P.sw;
  C.sh = P.sh;
  C.levels = P.n_levels;
  if (P.n_levels) {
    C.u0 = P.levels + P.off[0];
    C.w0 = P.lw[0];
    C.h0 = P.lh[0];
  }
  C.exposure = P.exposure;
  C.intensity = P.intensity;
  C.poison = P.poison;
  const dim3 grid(((P.sw + 1u) / 2u + 63u) / 64u, (P.sh + 3u) / 4u);
  if (P.auto_exposure) {
    if (P.tonemap == SVR_TONEMAP_CLAMP)
      hipLaunchKernelGGL(post_composite_auto_kernel<SVR_TONEMAP_CLAMP>, grid, block, 0, s, C, P.auto_exposure);
    else if (P.tonemap == SVR_TONEMAP_REINHARD)
      hipLaunchKernelGGL(post_composite_auto_kernel<SVR_TONEMAP_REINHARD>, grid, block, 0, s, C, P.auto_exposure);
    else
      hipLaunchKernelGGL(post_composite_auto_kernel<SVR_TONEMAP_ACES>, grid, block, 0, s, C, P.auto_exposure);
  } else if (P.tonemap == SVR_TONEMAP_CLAMP)
    hipLaunchKernelGGL(post_composite_kernel<SVR_TONEMAP_CLAMP>, grid, block, 0, s, C);
  else if (P.tonemap == SVR_TONEMAP_REINHARD)
    hipLaunchKernelGGL(post_composite_kernel<SVR_TONEMAP_REINHARD>, grid, block, 0, s, C);
  else
    hipLaunchKernelGGL(post_composite_kernel<SVR_TONEMAP_ACES>, grid, block, 0, s, C);
}

}  // namespace svr
