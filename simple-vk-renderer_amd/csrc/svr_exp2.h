// svr_exp2.h — the contract's 2^x, stated once for the kernels that need it (k_exposure.hip, k_fog.hip).
// No division and no square root in here: the header means the same in every file's build.
#pragma once

#include "svr_device.h"

namespace svr {

// C41: 2^x for |x| <= 16
__device__ __forceinline__ float exp2_poly(float x) {
  const float n = floorf(x), f = x - n;  // f in [0, 1], exact
  float p = 0x1.ca8f0ap-13f;
  p = fmaf(p, f, 0x1.44d4d2p-10f);
  p = fmaf(p, f, 0x1.3d54d8p-7f);
  p = fmaf(p, f, 0x1.c67f5p-5f);
  p = fmaf(p, f, 0x1.ebfdf2p-3f);
  p = fmaf(p, f, 0x1.62e428p-1f);
  p = fmaf(p, f, 1.0f);
  return __uint_as_float(__float_as_uint(p) + ((uint32_t)(int)n << 23));  // p in [1, 2.0000003]: the exponent takes n
}

}  // namespace svr
