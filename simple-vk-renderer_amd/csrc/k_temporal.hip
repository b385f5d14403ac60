// k_temporal.hip — temporal antialiasing (include/svr_temporal.h): the colour target resolved against a reprojected,
// neighbourhood-clamped history, in place.  Arithmetic: DESIGN.md C27-C31; the in-place hazard, ordering and the replay
// argument: DESIGN.md §5 "Temporal antialiasing".
//
// Two kernels (launch_temporal), because a workgroup's 3 x 3 window reaches into its neighbours' pixels: no kernel that
// reads a colour neighbourhood writes the colour target.
//   temporal_resolve_kernel   reads colour, depth and the old history, writes the new history only.  One workgroup of 256
//                             lanes per 32 x 32 tile of the scissor: the 34 x 34 window of san'd colour (fp32, a plane per
//                             channel) and of depth is staged into LDS at clamped coordinates, so the LDS image is the
//                             edge-clamped image and no tap needs a test; a lane then resolves 4 pixels of one column, the
//                             3 x 3 minimum, maximum and nearest depth taken separably (rows first, in registers).  The
//                             four history taps of a pixel are global gathers.
//   temporal_copy_kernel      the new history's RGB halves over the colour target's, alpha half kept: two pixels per lane
//                             (16 bytes) where the address allows, else one at a time.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch.  Both kernels read the
// context's poison flag first: after an overflow they write nothing.
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

namespace svr {

namespace {

constexpr uint32_t TT = 32;      // the tile of the scissor a workgroup resolves
constexpr uint32_t TS = TT + 2;  // ... and the staged texels per side: one more each way
constexpr uint32_t TP = 36;      // floats per staged row: window column c sits at index c + 1, so the texel pairs that
                                 // start at window column 1 (the tile's own first column) are 8-byte aligned in LDS

__device__ __forceinline__ float min2(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float max2(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float lerp(float t, float a, float b) { return fmaf(t, b - a, a); }

}  // namespace

__global__ __launch_bounds__(256) void temporal_resolve_kernel(TemporalLaunch A) {
  if (*A.poison) return;
  __shared__ __attribute__((aligned(16))) float s_c[3][TS][TP];  // san(I) at clamped coordinates
  __shared__ __attribute__((aligned(16))) float s_z[TS][TP];     // depth, likewise
  const uint32_t t = threadIdx.x;
  const uint32_t tx0 = blockIdx.x * TT, ty0 = blockIdx.y * TT;  // the tile's origin inside the scissor

  // ---- stage the window: per row the single column 0, sixteen pairs from column 1 on, the single column 33
  for (uint32_t i = t; i < TS * 18u; i += 256u) {
    const uint32_t wr = i / 18u, it = i - wr * 18u;
    const uint32_t y = A.sy + clamp_to((int)(ty0 + wr) - 1, A.sh);
    const uint2* crow = A.color + (size_t)y * A.W + A.sx;
    const float* zrow = A.depth + (size_t)y * A.W + A.sx;
    const bool pair = it >= 1u && it <= 16u;
    const uint32_t wc = it == 0u ? 0u : (it == 17u ? TS - 1u : 2u * it - 1u);
    const uint32_t xa = tx0 + wc - 1u;  // (window column 0 of tile 0 wraps; it is not a pair and is clamped below)
    if (pair && xa + 1u < A.sw && aligned_to(crow + xa, 16u) && aligned_to(zrow + xa, 8u)) {
      const uint4 q = *reinterpret_cast<const uint4*>(crow + xa);
      const float2 z = *reinterpret_cast<const float2*>(zrow + xa);
      const Rgb a = decode_rgb(make_uint2(q.x, q.y)), b = decode_rgb(make_uint2(q.z, q.w));
      *reinterpret_cast<float2*>(&s_c[0][wr][wc + 1u]) = make_float2(san(a.r), san(b.r));
      *reinterpret_cast<float2*>(&s_c[1][wr][wc + 1u]) = make_float2(san(a.g), san(b.g));
      *reinterpret_cast<float2*>(&s_c[2][wr][wc + 1u]) = make_float2(san(a.b), san(b.b));
      *reinterpret_cast<float2*>(&s_z[wr][wc + 1u]) = z;
    } else {
      for (uint32_t k = 0; k < (pair ? 2u : 1u); k++) {
        const uint32_t x = clamp_to((int)(tx0 + wc + k) - 1, A.sw);
        const Rgb q = decode_rgb(crow[x]);
        s_c[0][wr][wc + k + 1u] = san(q.r);
        s_c[1][wr][wc + k + 1u] = san(q.g);
        s_c[2][wr][wc + k + 1u] = san(q.b);
        s_z[wr][wc + k + 1u] = zrow[x];
      }
    }
  }
  __syncthreads();

  // ---- C27, C28: a lane takes column c, rows r0 .. r0 + 3 of the tile: the row-wise minimum, maximum and nearest depth of
  // the six window rows those pixels reach, once; the 32 lanes of a half wave read 32 consecutive floats
  const uint32_t c = t & 31u, r0 = 4u * (t >> 5);
  float hmn[3][6], hmx[3][6], hz[6], ctr[3][4];
#pragma unroll
  for (uint32_t j = 0; j < 6u; j++) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float* p = &s_c[ch][r0 + j][c + 1u];
      const float a = p[0], b = p[1], d = p[2];
      hmn[ch][j] = min2(min2(a, b), d);
      hmx[ch][j] = max2(max2(a, b), d);
      if (j >= 1u && j <= 4u) ctr[ch][j - 1u] = b;
    }
    const float* p = &s_z[r0 + j][c + 1u];
    hz[j] = max2(max2(p[0], p[1]), p[2]);
  }

  const uint32_t x = tx0 + c;
  if (x >= A.sw) return;
  const uint32_t px = A.sx + x;
  const float xn = pixel_ndc(px, A.two_over_w);
  const float x_lo = (float)A.sx, x_hi = (float)(A.sx + A.sw), y_lo = (float)A.sy, y_hi = (float)(A.sy + A.sh);
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t y = ty0 + r0 + i;
    if (y >= A.sh) break;
    const uint32_t py = A.sy + y;
    float cc[3], mn[3], mx[3], hist[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      cc[ch] = ctr[ch][i];
      mn[ch] = min2(min2(hmn[ch][i], hmn[ch][i + 1u]), hmn[ch][i + 2u]);
      mx[ch] = max2(max2(hmx[ch][i], hmx[ch][i + 1u]), hmx[ch][i + 2u]);
    }
    const float z = max2(max2(hz[i], hz[i + 1u]), hz[i + 2u]);
    // C29: the C0 chain, one matrix, no intermediate divide
    const Vec4 q = mat_vec(A.reproject, xn, pixel_ndc(py, A.two_over_h), z, 1.0f);  // (q.z is not used)
    bool valid = A.history_valid != 0u && q.w > 0.0f;
    if (valid) {
      const float r = rcp_ieee(q.w);
      const float hx = fmaf(q.x * r, A.half_w, A.half_w), hy = fmaf(q.y * r, A.half_h, A.half_h);
      valid = hx >= x_lo && hx < x_hi && hy >= y_lo && hy < y_hi;  // on the floats, before any conversion (NaN fails)
      if (valid) {
        // C30: hx - 0.5 lies in [sx - 0.5, sx + sw - 0.5), so the floors fit an int and the taps clamp into the scissor
        const float fx = hx - 0.5f, fy = hy - 0.5f;
        const float flx = floorf(fx), fly = floorf(fy);
        const float tx = fx - flx, ty = fy - fly;
        const uint32_t hx0 = A.sx + clamp_to((int)flx - (int)A.sx, A.sw), hx1 = A.sx + clamp_to((int)flx + 1 - (int)A.sx, A.sw);
        const uint32_t hy0 = A.sy + clamp_to((int)fly - (int)A.sy, A.sh), hy1 = A.sy + clamp_to((int)fly + 1 - (int)A.sy, A.sh);
        const uint2* h0 = A.hist_in + (size_t)hy0 * A.W;
        const uint2* h1 = A.hist_in + (size_t)hy1 * A.W;
        const uint2 q00 = h0[hx0], q10 = h0[hx1], q01 = h1[hx0], q11 = h1[hx1];
        const uint32_t w00[3] = {q00.x & 0xffffu, q00.x >> 16, q00.y & 0xffffu}, w10[3] = {q10.x & 0xffffu, q10.x >> 16, q10.y & 0xffffu};
        const uint32_t w01[3] = {q01.x & 0xffffu, q01.x >> 16, q01.y & 0xffffu}, w11[3] = {q11.x & 0xffffu, q11.x >> 16, q11.y & 0xffffu};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const float top = lerp(tx, half_bits_to_float(w00[ch]), half_bits_to_float(w10[ch]));
          const float bot = lerp(tx, half_bits_to_float(w01[ch]), half_bits_to_float(w11[ch]));
          hist[ch] = lerp(ty, top, bot);
        }
      }
    }
    // C31
    uint32_t o[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      float hc = hist[ch];
      if (A.clamp) {
        hc = hc < mn[ch] ? mn[ch] : hc;
        hc = hc > mx[ch] ? mx[ch] : hc;
      }
      o[ch] = h16((valid && A.blend < 1.0f) ? fmaf(A.blend, cc[ch] - hc, hc) : cc[ch]);
    }
    A.hist_out[(size_t)py * A.W + px] = make_uint2(o[0] | (o[1] << 16), o[2]);  // the fourth half is 0
  }
}

__global__ __launch_bounds__(256) void temporal_copy_kernel(TemporalLaunch A) {
  if (*A.poison) return;
  const uint32_t x = (blockIdx.x * 64u + (threadIdx.x & 63u)) * 2u, y = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (x >= A.sw || y >= A.sh) return;
  const size_t off = (size_t)(A.sy + y) * A.W + A.sx + x;
  uint2* at = A.color + off;
  const uint2* h = A.hist_out + off;
  if (x + 1u < A.sw && aligned_to(at, 16u) && aligned_to(h, 16u)) {
    const uint4 q = *reinterpret_cast<const uint4*>(at);
    const uint4 n = *reinterpret_cast<const uint4*>(h);
    *reinterpret_cast<uint4*>(at) = make_uint4(n.x, keep_alpha(n.y, q.y), n.z, keep_alpha(n.w, q.w));
  } else {
    at[0] = make_uint2(h[0].x, keep_alpha(h[0].y, at[0].y));
    if (x + 1u < A.sw) at[1] = make_uint2(h[1].x, keep_alpha(h[1].y, at[1].y));
  }
}

void launch_temporal(const TemporalLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 block(256);
  hipLaunchKernelGGL(temporal_resolve_kernel, dim3((A.sw + TT - 1u) / TT, (A.sh + TT - 1u) / TT), block, 0, s, A);
  hipLaunchKernelGGL(temporal_copy_kernel, dim3(((A.sw + 1u) / 2u + 63u) / 64u, (A.sh + 3u) / 4u), block, 0, s, A);
}

}  // namespace svr
