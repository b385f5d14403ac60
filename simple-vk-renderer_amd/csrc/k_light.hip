// k_light.hip — the deferred lighting pass (include/svr_lighting.h): a shadowed sun and tiled point lights over the
// G-buffer.  Arithmetic: DESIGN.md C17-C20; the culling argument: DESIGN.md §5 "Deferred lighting".
//
// One workgroup of 256 lanes per 32 x 32 tile of the pass's tile grid (the grid of the geometry passes: tile rows are
// owned under svr_set_row_interleave).  Lane t holds the four pixels (4 (t & 7) .. + 3, t >> 3) of the tile: one 16-byte
// load of depth where the row allows it, four each of normal and albedo.
//   1  positions (C17) of the lane's winner pixels; the tile's box of the finite ones: wave reductions, then LDS.
//      A tile without a winner exits.
//   2  lanes stride over the lights; a light whose sphere meets the box sets its bit of a 4096-bit LDS mask.
//   3  every pixel starts from the sun (C18: one shadow texel), then the mask is walked in ascending bit order — the
//      walk is uniform over the workgroup, so a light's record is a scalar load — and the colour is encoded and stored (C20).
// light_ao_kernel is the same body with the ambient term scaled by the ambient target's texel (include/svr_ambient.h).
// Ordinary vector stores only; nothing is handed between workgroups.  The kernel reads the context's poison flag first:
// after an overflow it writes nothing.
#include <hip/hip_fp16.h>

#include "svr_launch.h"

namespace svr {

constexpr uint32_t LIGHT_WORDS = SVR_MAX_LIGHTS / 32u;
constexpr uint32_t WINNER_BITS = 0x3F800000u;  // the albedo texel's w of an opaque winner (include/svr_attributes.h)

struct Vec4 {
  float x, y, z, w;
};

// matrix (column-major) times vector, the C0 chain
__device__ __forceinline__ Vec4 mat_vec(const float* m, float x, float y, float z, float w) {
  Vec4 r;
  r.x = m[0] * x; r.y = m[1] * x; r.z = m[2] * x; r.w = m[3] * x;
  r.x = fmaf(m[4], y, r.x); r.y = fmaf(m[5], y, r.y); r.z = fmaf(m[6], y, r.z); r.w = fmaf(m[7], y, r.w);
  r.x = fmaf(m[8], z, r.x); r.y = fmaf(m[9], z, r.y); r.z = fmaf(m[10], z, r.z); r.w = fmaf(m[11], z, r.w);
  r.x = fmaf(m[12], w, r.x); r.y = fmaf(m[13], w, r.y); r.z = fmaf(m[14], w, r.z); r.w = fmaf(m[15], w, r.w);
  return r;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return (f2u(x) & 0x7f800000u) != 0x7f800000u && (f2u(y) & 0x7f800000u) != 0x7f800000u && (f2u(z) & 0x7f800000u) != 0x7f800000u;
}

// C20: the stores of C10.  fp16: the fp32 value is pinned in a VGPR so that "fma -> cvt" is not fused into one rounding
// (the tile kernel's codec does the same).
__device__ __forceinline__ float pin(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint2 encode16(float r, float g, float b) {
  const uint32_t hr = __half_as_ushort(__float2half_rn(pin(r))), hg = __half_as_ushort(__float2half_rn(pin(g)));
  const uint32_t hb = __half_as_ushort(__float2half_rn(pin(b)));
  return make_uint2(hr | (hg << 16), hb | (0x3c00u << 16));
}
__device__ __forceinline__ uint32_t un8(float f) { return (uint32_t)__float2int_rn(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ uint32_t encode8(float r, float g, float b) { return un8(r) | (un8(g) << 8) | (un8(b) << 16) | (255u << 24); }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// light_kernel<FMT>, and light_ao_kernel<FMT> with the ambient factor: one body (k_light_body.h)
#define SVR_LIGHT_KERNEL light_kernel
#define SVR_LIGHT_AO 0
#include "k_light_body.h"
#undef SVR_LIGHT_KERNEL
#undef SVR_LIGHT_AO
#define SVR_LIGHT_KERNEL light_ao_kernel
#define SVR_LIGHT_AO 1
#include "k_light_body.h"
#undef SVR_LIGHT_KERNEL
#undef SVR_LIGHT_AO

void launch_light(const LightLaunch& L, int color_format, uint32_t tiles_y, hipStream_t s) {
  if (L.tiles_x == 0u || tiles_y == 0u) return;
  const dim3 grid(L.tiles_x, tiles_y), block(256);
  if (L.ao) {
    if (color_format == SVR_COLOR_RGBA16F)
      hipLaunchKernelGGL(light_ao_kernel<SVR_COLOR_RGBA16F>, grid, block, 0, s, L);
    else
      hipLaunchKernelGGL(light_ao_kernel<SVR_COLOR_RGBA8>, grid, block, 0, s, L);
  } else if (color_format == SVR_COLOR_RGBA16F)
    hipLaunchKernelGGL(light_kernel<SVR_COLOR_RGBA16F>, grid, block, 0, s, L);
  else
    hipLaunchKernelGGL(light_kernel<SVR_COLOR_RGBA8>, grid, block, 0, s, L);
}

}  // namespace svr
