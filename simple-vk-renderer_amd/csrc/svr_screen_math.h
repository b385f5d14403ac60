// svr_screen_math.h — what the screen-space passes compute alike: a pixel centre in NDC, the world
// position behind a depth texel, and the shadow-map lookup.  Stated once: a kernel file includes this header and
// restates none of it.  The only reciprocal in here is svr_device.h's rcp_ieee (C3).  The two steps of C17 are composed
// where they are used, point_of(unproject(..)): one function of both is optimised on its own before it is inlined and
// leaves the kernels another instruction order (profiles/screen_math_isa.txt).
#pragma once

#include "svr_launch.h"

namespace svr {

// C17: the centre of pixel p of an axis in NDC; two_over = 2.0f / float(extent), divided once, on the host
__device__ __forceinline__ float pixel_ndc(uint32_t p, float two_over) { return fmaf((float)p + 0.5f, two_over, -1.0f); }

// C17 in two steps, for the caller that looks at h.w before it divides: the homogeneous position of (xn, yn, z) ...
__device__ __forceinline__ Vec4 unproject(const float* inv_viewproj, float xn, float yn, float z) { return mat_vec(inv_viewproj, xn, yn, z, 1.0f); }
// ... and the point, h.xyz * (1 / h.w)
struct Point {
  float x, y, z;
};
__device__ __forceinline__ Point point_of(Vec4 h) {
  const float rw = rcp_ieee(h.w);
  return {h.x * rw, h.y * rw, h.z * rw};
}

// C18's lookup for q = S.viewproj * (p, 1): is p behind what the map holds?  Outside the map or behind the light: no.
// The caller tests S.depth first: without a map nothing here is read.
__device__ __forceinline__ bool shadow_occluded(const ShadowMap& S, float qx, float qy, float qz, float qw) {
  const float rq = rcp_ieee(qw);
  const float sx = fmaf(qx * rq, S.half_w, S.half_w), sy = fmaf(qy * rq, S.half_h, S.half_h);
  const float sz = qz * rq;
  const float fx = floorf(sx), fy = floorf(sy);
  // (the extents are at most 2^24, so they are exact as floats and a passing floor is an index inside the map)
  bool occluded = false;
  if (qw > 0.0f && fx >= 0.0f && fx < (float)S.w && fy >= 0.0f && fy < (float)S.h)
    occluded = sz + S.bias < S.depth[(size_t)(uint32_t)fy * S.w + (uint32_t)fx];
  return occluded;
}

}  // namespace svr
