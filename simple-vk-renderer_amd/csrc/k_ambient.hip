// k_ambient.hip — screen-space ambient occlusion (include/svr_ambient.h): the ambient factor of every pixel of the scissor
// from the depth target and the normal plane.  Arithmetic: DESIGN.md C32-C37; the bounds, the choice of what is staged and
// the replay argument: DESIGN.md §5 "Ambient occlusion".
//
// Two kernels (launch_ambient), because the blur of a pixel reads the raw values of its neighbours' workgroups:
//   ambient_raw_kernel    reads depth and normal, writes the (a, 1/w) scratch plane.  One workgroup of 256 lanes per
//                         32 x 32 tile of the scissor: the 64 x 64 window of depth the tile's taps can reach (16 each way)
//                         is staged into LDS, 16 bytes a lane where the row allows, with 0 for every texel outside the
//                         scissor — a depth of 0 contributes nothing (C34), so the LDS image is the edge-tested image
//                         and no tap needs a test of its own.  A lane then takes 4 pixels of one column: the centre's
//                         position and normal, and eight scattered depths out of LDS, each unprojected in full (C17, C35).
//   ambient_blur_kernel   stages the 36 x 36 window of the scratch plane at clamped coordinates, takes the 25 taps out of
//                         LDS (C37) and stores the ambient target; under SVR_AMBIENT_NO_BLUR it copies a.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch, and neither kernel reads a
// plane the same launch writes.  Both kernels read the context's poison flag first: after an overflow they write nothing.
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

#define SVR_AMBIENT_TABLE __device__ const
#include "svr_ambient_tables.h"

namespace svr {

namespace {

constexpr uint32_t AT = 32;                     // the tile of the scissor a workgroup takes
constexpr int REACH = SVR_AMBIENT_MAX_REACH;    // C34: |ox|, |oy| <= REACH
constexpr uint32_t AW = AT + 2u * REACH;        // the staged depth window, per side
constexpr uint32_t BR = 2;                      // the blur's reach
constexpr uint32_t BW = AT + 2u * BR;           // the staged raw window, per side

__device__ __forceinline__ int clamp_reach(int v) { return v < -REACH ? -REACH : (v > REACH ? REACH : v); }

}  // namespace

__global__ __launch_bounds__(256) void ambient_raw_kernel(AmbientLaunch A) {
  if (*A.poison) return;
  __shared__ __attribute__((aligned(16))) float s_z[AW][AW];  // depth; 0 outside the scissor
  const uint32_t t = threadIdx.x;
  const uint32_t tx0 = blockIdx.x * AT, ty0 = blockIdx.y * AT;  // the tile's origin inside the scissor

  // ---- stage the window: 64 rows of sixteen groups of four texels; (x, y) are coordinates inside the scissor
  for (uint32_t i = t; i < AW * (AW / 4u); i += 256u) {
    const uint32_t wr = i / (AW / 4u), wc = (i % (AW / 4u)) * 4u;
    const int y = (int)(ty0 + wr) - REACH, x = (int)(tx0 + wc) - REACH;
    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (y >= 0 && (uint32_t)y < A.sh) {
      const float* row = A.depth + (size_t)(A.sy + (uint32_t)y) * A.W + A.sx;
      if (x >= 0 && (uint32_t)x + 3u < A.sw && aligned_to(row + x, 16u)) {
        const float4 v = *reinterpret_cast<const float4*>(row + x);
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (x + k >= 0 && (uint32_t)(x + k) < A.sw) q[k] = row[x + k];
      }
    }
    *reinterpret_cast<float4*>(&s_z[wr][wc]) = make_float4(q[0], q[1], q[2], q[3]);
  }
  __syncthreads();

  // ---- a lane takes column c, rows r0 .. r0 + 3 of the tile: the 32 lanes of a half wave read and write consecutive texels
  const uint32_t c = t & 31u, r0 = 4u * (t >> 5);
  const uint32_t x = tx0 + c;
  if (x >= A.sw) return;
  const uint32_t px = A.sx + x;
  const float xn = pixel_ndc(px, A.two_over_w);
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t y = ty0 + r0 + i;
    if (y >= A.sh) break;
    const uint32_t py = A.sy + y;
    const size_t at = (size_t)py * A.W + px;
    // C32
    const float z = s_z[r0 + i + REACH][c + REACH];
    const float4 n = A.normal[at];
    const Vec4 h = unproject(A.inv_viewproj, xn, pixel_ndc(py, A.two_over_h), z);  // C17's first step: h.w is looked at below
    const float nn = fmaf(n.z, n.z, fmaf(n.y, n.y, n.x * n.x));
    if (!(z > 0.0f && f2u(n.w) != 0u && nn > 0.0f)) {
      A.raw[at] = make_float2(1.0f, 0.0f);
      continue;
    }
    // C33
    float rpx = A.radius_px * h.w;
    rpx = rpx < (float)REACH ? rpx : (float)REACH;
    if (!(rpx >= 1.0f)) {
      A.raw[at] = make_float2(1.0f, h.w);
      continue;
    }
    const Point P = point_of(h);
    // `/` and sqrtf are correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
    const float rl = 1.0f / sqrtf(nn);
    const float nx = n.x * rl, ny = n.y * rl, nz = n.z * rl;
    const uint32_t j = (py & 3u) * 4u + (px & 3u);
    const float rc = SVR_AMBIENT_R[j][0], rs = SVR_AMBIENT_R[j][1];
    float sum = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)SVR_AMBIENT_TAPS; k++) {
      // C34: 1 <= rpx <= 16, f < 1 and |u| <= 1 + 2 ulp, so the offsets are integers of at most 16 either way; the clamp
      // holds the index inside the window whatever the floats are
      const float dx = SVR_AMBIENT_D[k][0], dy = SVR_AMBIENT_D[k][1];
      const float ux = dx * rc - dy * rs, uy = fmaf(dx, rs, dy * rc);
      const float f = ((float)((3u * k) & 7u) + 0.5f) * 0.125f;
      const float rf = rpx * f;
      const int ox = clamp_reach((int)rintf(rf * ux)), oy = clamp_reach((int)rintf(rf * uy));
      if ((ox | oy) == 0) continue;
      const float zt = s_z[(int)(r0 + i) + REACH + oy][(int)c + REACH + ox];
      if (!(zt > 0.0f)) continue;  // a cleared texel, or one outside the scissor
      // C35: the tap's own position, in full
      // (two things stay spelled here, profiles/screen_math_isa.txt: the tap's coordinate is an int, whose conversion is
      // not pixel_ndc's instruction, and C17's second step, each product next to its difference)
      const float xt = fmaf((float)((int)px + ox) + 0.5f, A.two_over_w, -1.0f);
      const float yt = fmaf((float)((int)py + oy) + 0.5f, A.two_over_h, -1.0f);
      const Vec4 g = unproject(A.inv_viewproj, xt, yt, zt);
      const float gw = rcp_ieee(g.w);
      const float vx = g.x * gw - P.x, vy = g.y * gw - P.y, vz = g.z * gw - P.z;
      const float vv = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
      if (!(vv < A.radius2)) continue;
      const float vn = fmaf(vz, nz, fmaf(vy, ny, vx * nx)) - A.bias;
      sum = sum + (vn > 0.0f ? vn : 0.0f) / (vv + 0.0001f);
    }
    // C36
    float a = 1.0f - A.coef * sum;
    a = a > 0.0f ? a : 0.0f;
    A.raw[at] = make_float2(a, h.w);
  }
}

__global__ __launch_bounds__(256) void ambient_blur_kernel(AmbientLaunch A) {
  if (*A.poison) return;
  __shared__ float s_a[BW][BW], s_w[BW][BW];  // the raw plane's a and 1/w at coordinates clamped into the scissor
  const uint32_t t = threadIdx.x;
  const uint32_t tx0 = blockIdx.x * AT, ty0 = blockIdx.y * AT;
  const uint32_t c = t & 31u, r0 = 4u * (t >> 5);
  const uint32_t x = tx0 + c;
  if (!A.blur) {  // uniform
    if (x >= A.sw) return;
    for (uint32_t i = 0; i < 4u; i++) {
      const uint32_t y = ty0 + r0 + i;
      if (y >= A.sh) break;
      const size_t at = (size_t)(A.sy + y) * A.W + A.sx + x;
      A.out[at] = A.raw[at].x;
    }
    return;
  }
  for (uint32_t i = t; i < BW * BW; i += 256u) {
    const uint32_t wr = i / BW, wc = i - wr * BW;
    const uint32_t yy = A.sy + clamp_to((int)(ty0 + wr) - (int)BR, A.sh), xx = A.sx + clamp_to((int)(tx0 + wc) - (int)BR, A.sw);
    const float2 q = A.raw[(size_t)yy * A.W + xx];
    s_a[wr][wc] = q.x;
    s_w[wr][wc] = q.y;
  }
  __syncthreads();
  if (x >= A.sw) return;
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t y = ty0 + r0 + i;
    if (y >= A.sh) break;
    // C37
    const float hc = s_w[r0 + i + BR][c + BR];
    float o = 1.0f;
    if (f2u(hc) != 0u) {
      const float lim = A.sharpness * hc;
      float sum = 0.0f;
      uint32_t count = 0;
#pragma unroll
      for (uint32_t dy = 0; dy < 5u; dy++) {
#pragma unroll
        for (uint32_t dx = 0; dx < 5u; dx++) {
          const float ht = s_w[r0 + i + dy][c + dx], a = s_a[r0 + i + dy][c + dx];
          if ((dy == BR && dx == BR) || fabsf(ht - hc) <= lim) {
            sum = sum + a;
            count++;
          }
        }
      }
      o = sum / (float)count;
    }
    A.out[(size_t)(A.sy + y) * A.W + A.sx + x] = o;
  }
}

void launch_ambient(const AmbientLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 grid((A.sw + AT - 1u) / AT, (A.sh + AT - 1u) / AT), block(256);
  hipLaunchKernelGGL(ambient_raw_kernel, grid, block, 0, s, A);
  hipLaunchKernelGGL(ambient_blur_kernel, grid, block, 0, s, A);
}

}  // namespace svr
