// k_fog.hip — the fog pass (include/svr_fog.h): height fog and sun shafts marched through the shadow map at half
// resolution, composited over the RGBA16F colour target with a depth-aware upsample, in place.  Arithmetic: DESIGN.md
// C55-C60; ordering and the exactly-once argument: DESIGN.md §5 "Fog pass".
//
// Two kernels (launch_fog):
//   fog_march_kernel<SHADOW>   one lane per 2 x 2 block of the scissor; a workgroup of 256 lanes is a 32 x 8 patch of
//                              blocks, so the rays of a wave stay close in the shadow map.  A lane reads its block's
//                              depths, sets its ray up once (direction, length, dither, phase, and the shadow matrix
//                              applied to origin and direction), then walks the steps: two 2^x polynomials, and with
//                              SHADOW four fma, a reciprocal and one texel of the map.  It stores (S, T) and t_end.
//   fog_composite_kernel       one workgroup of 256 lanes per 32 x 16 tile of the scissor.  The 18 x 10 blocks the
//                              tile's taps can reach are staged in LDS at clamped coordinates, so the arrays hold the
//                              edge-clamped image and no tap needs a test.  A lane takes two pixels: one 16-byte load
//                              and store where the pair is aligned and inside the scissor, else one pixel at a time.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch (the composite reads what
// the march's launch wrote, in stream order).  Both kernels read the context's poison flag first: after an overflow they
// write nothing.
#include "svr_exp2.h"
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

namespace svr {

namespace {

constexpr float LOG2E = 0x1.715476p+0f;
constexpr float FOUR_PI = 0x1.921fb6p+3f;
constexpr uint32_t CT_W = 32, CT_H = 16;          // the composite's tile of pixels
constexpr uint32_t CS_W = CT_W / 2 + 2, CS_H = CT_H / 2 + 2;  // ... and the blocks staged for it

// C55: t(pixel), the distance from the camera to the pixel's C17 position, at most max_distance; a cleared depth texel
// (bits 0) and a distance that is no number count as max_distance.  x, y: the pixel in the target.
__device__ __forceinline__ float pixel_t(const FogLaunch& A, uint32_t x, uint32_t y, float z) {
  if (f2u(z) == 0u) return A.max_distance;
  // (C17's second step is spelled here and below, each product next to its difference: through point_of the compiler
  // schedules the three products otherwise, profiles/screen_math_isa.txt)
  const Vec4 h = unproject(A.inv_viewproj, pixel_ndc(x, A.two_over_w), pixel_ndc(y, A.two_over_h), z);
  const float rw = rcp_ieee(h.w);
  const float vx = h.x * rw - A.cam[0], vy = h.y * rw - A.cam[1], vz = h.z * rw - A.cam[2];
  // sqrtf is correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
  const float t = sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
  return t < A.max_distance ? t : A.max_distance;
}

// C56: the dither's hash
__device__ __forceinline__ uint32_t fog_hash(uint32_t bx, uint32_t by, uint32_t frame) {
  uint32_t h = (bx * 0x9E3779B1u) ^ (by * 0x85EBCA77u) ^ (frame * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// C41's argument, NaN included, into [lo, hi]
__device__ __forceinline__ float into(float x, float lo, float hi) {
  x = x > lo ? x : lo;
  return x < hi ? x : hi;
}

}  // namespace

template <bool SHADOW>
__global__ __launch_bounds__(256) void fog_march_kernel(FogLaunch A) {
  if (*A.poison) return;
  const uint32_t t = threadIdx.x;
  const uint32_t bx = blockIdx.x * 32u + (t & 31u), by = blockIdx.y * 8u + (t >> 5);
  if (bx >= A.gw || by >= A.gh) return;
  // ---- C55: the block's pixels and the ray
  const uint32_t x0 = A.sx + 2u * bx, y0 = A.sy + 2u * by;  // inside the scissor
  const bool two_x = 2u * bx + 1u < A.sw, two_y = 2u * by + 1u < A.sh;
  const float* d0 = A.depth + (size_t)y0 * A.W + x0;
  float m = pixel_t(A, x0, y0, d0[0]);
  if (two_x) {
    const float v = pixel_t(A, x0 + 1u, y0, d0[1]);
    m = v > m ? v : m;
  }
  if (two_y) {
    const float* d1 = d0 + A.W;
    float v = pixel_t(A, x0, y0 + 1u, d1[0]);
    m = v > m ? v : m;
    if (two_x) {
      v = pixel_t(A, x0 + 1u, y0 + 1u, d1[1]);
      m = v > m ? v : m;
    }
  }
  const float t_end = m;
  float dx, dy, dz;
  {
    // (the block's centre, not a pixel's: + 1.0f)
    const float xn = fmaf((float)x0 + 1.0f, A.two_over_w, -1.0f), yn = fmaf((float)y0 + 1.0f, A.two_over_h, -1.0f);
    const Vec4 h = unproject(A.inv_viewproj, xn, yn, 1.0f);
    const float rw = rcp_ieee(h.w);
    const float vx = h.x * rw - A.cam[0], vy = h.y * rw - A.cam[1], vz = h.z * rw - A.cam[2];
    // `/` and sqrtf are correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
    const float inv = 1.0f / sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
    dx = vx * inv; dy = vy * inv; dz = vz * inv;
  }
  // ---- C56, C57: the step and the dither
  const float delta = t_end / (float)A.steps;
  const float o = (float)(fog_hash(bx, by, A.frame) >> 24) * 0x1p-8f;
  // ---- C58: the phase, and the two sources a sample can see
  const float c = fmaf(dz, A.sun[2], fmaf(dy, A.sun[1], dx * A.sun[0]));
  const float x = fmaf(A.minus_2g, c, A.one_plus_g2);
  const float ph = A.one_minus_g2 / (FOUR_PI * (x * sqrtf(x)));
  const float lit_r = fmaf(A.sun_color[0], ph, A.fog_color[0]), lit_g = fmaf(A.sun_color[1], ph, A.fog_color[1]),
              lit_b = fmaf(A.sun_color[2], ph, A.fog_color[2]);
  const float dark_r = fmaf(A.sun_color[0], 0.0f, A.fog_color[0]), dark_g = fmaf(A.sun_color[1], 0.0f, A.fog_color[1]),
              dark_b = fmaf(A.sun_color[2], 0.0f, A.fog_color[2]);
  // the shadow matrix, applied once: to the origin as a point, to the direction as a vector
  Vec4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, dq = {0.0f, 0.0f, 0.0f, 0.0f};
  if (SHADOW) {
    const float* M = A.shadow.viewproj;
    q0 = mat_vec(M, A.cam[0], A.cam[1], A.cam[2], 1.0f);
    dq.x = fmaf(M[8], dz, fmaf(M[4], dy, M[0] * dx));
    dq.y = fmaf(M[9], dz, fmaf(M[5], dy, M[1] * dx));
    dq.z = fmaf(M[10], dz, fmaf(M[6], dy, M[2] * dx));
    dq.w = fmaf(M[11], dz, fmaf(M[7], dy, M[3] * dx));
  }
  // ---- C57: the march
  float Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, T = 1.0f;
#pragma unroll 2
  for (uint32_t i = 0; i < A.steps; i++) {
    const float ti = ((float)i + o) * delta;
    const float yi = fmaf(ti, dy, A.cam[1]);
    const float sigma = A.density * exp2_poly(into((A.height_base - yi) * A.kh, -16.0f, 16.0f));
    const float a = exp2_poly(into((sigma * delta) * -LOG2E, -16.0f, 0.0f));
    bool shadowed = false;
    if (SHADOW) {  // C18's lookup at the sample
      const float qx = fmaf(ti, dq.x, q0.x), qy = fmaf(ti, dq.y, q0.y), qz = fmaf(ti, dq.z, q0.z), qw = fmaf(ti, dq.w, q0.w);
      shadowed = shadow_occluded(A.shadow, qx, qy, qz, qw);
    }
    const float w = T * (1.0f - a);
    Sr = fmaf(w, shadowed ? dark_r : lit_r, Sr);
    Sg = fmaf(w, shadowed ? dark_g : lit_g, Sg);
    Sb = fmaf(w, shadowed ? dark_b : lit_b, Sb);
    T = T * a;
  }
  const size_t at = (size_t)by * A.gw + bx;
  A.st[at] = make_float4(Sr, Sg, Sb, T);
  A.te[at] = t_end;
}

namespace {

// C59, C60 for one pixel.  (x, y): the pixel in the scissor; s_st / s_te: the staged blocks, (hx0, hy0) the grid
// coordinates of their first (which may be -1: the arrays hold the clamped image)
__device__ __forceinline__ uint2 fog_pixel(const FogLaunch& A, uint2 texel, float z, uint32_t x, uint32_t y, const float4 (*s_st)[CS_W],
                                           const float (*s_te)[CS_W], int hx0, int hy0) {
  const float tp = pixel_t(A, A.sx + x, A.sy + y, z);
  const float u = fmaf((float)x, 0.5f, -0.25f), v = fmaf((float)y, 0.5f, -0.25f);
  const float flx = floorf(u), fly = floorf(v);
  const float tx = u - flx, ty = v - fly;  // 0.25 or 0.75
  const int cx = (int)flx - hx0, cy = (int)fly - hy0;
  const float b[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
  float nr = 0.0f, ng = 0.0f, nb = 0.0f, nt = 0.0f, den = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = cx + (k & 1), r = cy + (k >> 1);
    const float4 s = s_st[r][c];
    // `/` is correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
    const float w = b[k] / fmaf(A.edge, fabsf(s_te[r][c] - tp), 1.0f);
    if (k == 0) {
      nr = w * s.x; ng = w * s.y; nb = w * s.z; nt = w * s.w; den = w;
    } else {
      nr = fmaf(w, s.x, nr); ng = fmaf(w, s.y, ng); nb = fmaf(w, s.z, nb); nt = fmaf(w, s.w, nt); den = den + w;
    }
  }
  const float rd = 1.0f / den;
  const float Sr = nr * rd, Sg = ng * rd, Sb = nb * rd, T = nt * rd;
  const Rgb in = decode_rgb(texel);
  return encode_rgb({san(fmaf(in.r, T, Sr)), san(fmaf(in.g, T, Sg)), san(fmaf(in.b, T, Sb))}, texel);
}

}  // namespace

__global__ __launch_bounds__(256) void fog_composite_kernel(FogLaunch A) {
  if (*A.poison) return;
  __shared__ float4 s_st[CS_H][CS_W];
  __shared__ float s_te[CS_H][CS_W];
  const uint32_t t = threadIdx.x;
  const int hx0 = (int)(blockIdx.x * (CT_W / 2u)) - 1, hy0 = (int)(blockIdx.y * (CT_H / 2u)) - 1;
  if (t < CS_W * CS_H) {
    const uint32_t r = t / CS_W, c = t - r * CS_W;
    const size_t at = (size_t)clamp_to(hy0 + (int)r, A.gh) * A.gw + clamp_to(hx0 + (int)c, A.gw);
    s_st[r][c] = A.st[at];
    s_te[r][c] = A.te[at];
  }
  __syncthreads();
  const uint32_t x = blockIdx.x * CT_W + 2u * (t & 15u), y = blockIdx.y * CT_H + (t >> 4);
  if (x >= A.sw || y >= A.sh) return;
  const size_t at = (size_t)(A.sy + y) * A.W + A.sx + x;
  uint2* px = A.color + at;
  const float* dz = A.depth + at;
  if (x + 1u < A.sw && aligned_to(px, 16u)) {
    const uint4 q = *reinterpret_cast<const uint4*>(px);
    const float za = dz[0], zb = dz[1];  // (a caller's depth target need not share the colour target's alignment)
    const uint2 a = fog_pixel(A, make_uint2(q.x, q.y), za, x, y, s_st, s_te, hx0, hy0);
    const uint2 b = fog_pixel(A, make_uint2(q.z, q.w), zb, x + 1u, y, s_st, s_te, hx0, hy0);
    *reinterpret_cast<uint4*>(px) = make_uint4(a.x, a.y, b.x, b.y);
  } else {
    px[0] = fog_pixel(A, px[0], dz[0], x, y, s_st, s_te, hx0, hy0);
    if (x + 1u < A.sw) px[1] = fog_pixel(A, px[1], dz[1], x + 1u, y, s_st, s_te, hx0, hy0);
  }
}

void launch_fog(const FogLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 block(256);
  const dim3 march((A.gw + 31u) / 32u, (A.gh + 7u) / 8u);
  if (A.shadow.depth)
    hipLaunchKernelGGL(fog_march_kernel<true>, march, block, 0, s, A);
  else
    hipLaunchKernelGGL(fog_march_kernel<false>, march, block, 0, s, A);
  hipLaunchKernelGGL(fog_composite_kernel, dim3((A.sw + CT_W - 1u) / CT_W, (A.sh + CT_H - 1u) / CT_H), block, 0, s, A);
}

}  // namespace svr
