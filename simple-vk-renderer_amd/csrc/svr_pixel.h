// svr_pixel.h — how a kernel reads and writes a render target's texels, the RGB rewrite of the
// in-place HDR passes among it, and the two small index helpers every screen-space pass needs.  Stated once: a kernel file includes this header and restates none of it.
// There is no division and no square root in here, so the header means the same in the files built with
// -fhip-fp32-correctly-rounded-divide-sqrt and in those built without.
#pragma once

#include <hip/hip_fp16.h>

#include "svr_device.h"

namespace svr {

// ---- fp16 (RGBA16F targets, the bloom levels, the temporal history)
// The store rule: the fp32 result must exist before it is rounded to fp16 (two roundings, as an attachment store after
// an fp32 shader does).  Without the barrier hipcc fuses "fma -> cvt" into v_fma_mixlo_f16, which rounds once and
// differs from the contract on fp16 ties.  pin() is that barrier: the value passes through a VGPR.
__device__ __forceinline__ float pin(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint32_t h16(float x) { return __half_as_ushort(__float2half_rn(pin(x))); }
__device__ __forceinline__ float half_bits_to_float(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }

constexpr float HALF_MAX = 65504.0f;
// what an HDR pass takes a stored half for: NaN and negatives are 0, +inf is the largest half
__device__ __forceinline__ float san(float v) { return v > 0.0f ? (v < HALF_MAX ? v : HALF_MAX) : 0.0f; }

// ---- the in-place HDR passes over an RGBA16F target: RGB halves in, RGB halves out, the alpha half as it was
struct Rgb {
  float r, g, b;
};
__device__ __forceinline__ Rgb decode_rgb(uint2 t) { return {half_bits_to_float(t.x & 0xffffu), half_bits_to_float(t.x >> 16), half_bits_to_float(t.y & 0xffffu)}; }
// a texel's second word: the blue half of b_word, the alpha half of old_word
__device__ __forceinline__ uint32_t keep_alpha(uint32_t b_word, uint32_t old_word) { return (b_word & 0xffffu) | (old_word & 0xffff0000u); }
__device__ __forceinline__ uint2 encode_rgb(Rgb c, uint2 old) { return make_uint2(h16(c.r) | (h16(c.g) << 16), keep_alpha(h16(c.b), old.y)); }

// ---- unorm8 (RGBA8 targets, the swapchain, texels)
constexpr float kInv255 = 0x1.010102p-8f;
__device__ __forceinline__ uint32_t un8(float f) { return (uint32_t)__float2int_rn(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ float chan(uint32_t t, int c) { return (float)((t >> (8 * c)) & 0xffu) * kInv255; }

// ---- colour target codecs: the attachment holds fp16 (reference) or unorm8
template <int FMT>
struct Codec;
template <>
struct Codec<SVR_COLOR_RGBA16F> {
  typedef uint2 enc_t;
  // four pins, then the four round-to-nearest-even conversions as the two pairs the words hold, (r, g) and (b, a): a
  // packed conversion leaves each word as it is stored, nothing is shifted or ORed together afterwards
  static __device__ __forceinline__ enc_t encode(float4 c) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    c.x = pin(c.x); c.y = pin(c.y); c.z = pin(c.z); c.w = pin(c.w);
    const f16x2 rg = __builtin_convertvector((f32x2){c.x, c.y}, f16x2), ba = __builtin_convertvector((f32x2){c.z, c.w}, f16x2);
    return make_uint2(__builtin_bit_cast(uint32_t, rg), __builtin_bit_cast(uint32_t, ba));
  }
  static __device__ __forceinline__ float4 decode(enc_t e) {
    return make_float4(half_bits_to_float(e.x & 0xffffu), half_bits_to_float(e.x >> 16), half_bits_to_float(e.y & 0xffffu),
                       half_bits_to_float(e.y >> 16));
  }
};
template <>
struct Codec<SVR_COLOR_RGBA8> {
  typedef uint32_t enc_t;
  static __device__ __forceinline__ enc_t encode(float4 c) { return un8(c.x) | (un8(c.y) << 8) | (un8(c.z) << 16) | (un8(c.w) << 24); }
  static __device__ __forceinline__ float4 decode(enc_t e) { return make_float4(chan(e, 0), chan(e, 1), chan(e, 2), chan(e, 3)); }
};

// ---- indices
// n: a power of two
__device__ __forceinline__ bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1u)) == 0u; }
// v clamped into [0, n - 1]
__device__ __forceinline__ uint32_t clamp_to(int v, uint32_t n) { return v < 0 ? 0u : ((uint32_t)v > n - 1u ? n - 1u : (uint32_t)v); }

}  // namespace svr
