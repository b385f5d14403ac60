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
// light_kernel<FMT, true> scales the ambient term by the ambient target's texel (include/svr_ambient.h).
// Ordinary vector stores only; nothing is handed between workgroups.  The kernel reads the context's poison flag first:
// after an overflow it writes nothing.
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

namespace svr {

constexpr uint32_t LIGHT_WORDS = SVR_MAX_LIGHTS / 32u;
constexpr uint32_t WINNER_BITS = 0x3F800000u;  // the albedo texel's w of an opaque winner (include/svr_attributes.h)

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return (f2u(x) & 0x7f800000u) != 0x7f800000u && (f2u(y) & 0x7f800000u) != 0x7f800000u && (f2u(z) & 0x7f800000u) != 0x7f800000u;
}

// C20: the stores of C10 (svr_pixel.h) with a constant alpha of 1, which is a literal: it was never a float to pin
__device__ __forceinline__ uint2 encode16(float r, float g, float b) {
  const uint32_t hr = h16(r), hg = h16(g), hb = h16(b);
  return make_uint2(hr | (hg << 16), hb | (0x3c00u << 16));
}
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

// AO: the ambient term of C18 is scaled by the ambient target's texel
template <int FMT, bool AO>
__global__ __launch_bounds__(256) void light_kernel(LightLaunch L) {
  if (*L.poison) return;
  __shared__ float s_box[4][6];
  __shared__ uint32_t s_any[4];
  __shared__ uint32_t s_mask[LIGHT_WORDS];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
  const uint32_t tile = blockIdx.y * L.tiles_x + blockIdx.x;
  const uint32_t x_end = L.sx + L.sw, y_end = L.sy + L.sh;
  const uint32_t px0 = L.sx + blockIdx.x * TILE + 4u * (t & 7u);
  const uint32_t py = L.sy + (blockIdx.y * L.rstride + L.roff) * TILE + (t >> 3);
  const bool row_in = py < y_end;
  const size_t at = (size_t)py * L.W + px0;  // (only used where the pixel is inside the scissor, hence the target)

  // ---- phase 1: the G-buffer of the lane's pixels, their positions, the tile's box
  bool win[4] = {false, false, false, false};
  float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float nx[4], ny[4], nz[4], cr[4], cg[4], cb[4], X[4], Y[4], Z[4];
  if (row_in) {
    if (px0 + 3u < x_end && (reinterpret_cast<uintptr_t>(L.depth + at) & 15u) == 0u) {
      const float4 q = *reinterpret_cast<const float4*>(L.depth + at);
      z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (px0 + k < x_end) z[k] = L.depth[at + k];
    }
  }
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const float yn = pixel_ndc(py, L.two_over_h);
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    nx[k] = ny[k] = nz[k] = cr[k] = cg[k] = cb[k] = X[k] = Y[k] = Z[k] = 0.0f;
    if (!row_in || px0 + k >= x_end) continue;
    const float4 a = L.albedo[at + k];
    if (f2u(a.w) != WINNER_BITS) continue;
    win[k] = true;
    const float4 n = L.normal[at + k];
    nx[k] = n.x; ny[k] = n.y; nz[k] = n.z;
    cr[k] = a.x; cg[k] = a.y; cb[k] = a.z;
    const Point p = point_of(unproject(L.inv_viewproj, pixel_ndc(px0 + k, L.two_over_w), yn, z[k]));  // C17
    X[k] = p.x; Y[k] = p.y; Z[k] = p.z;
    if (finite3(X[k], Y[k], Z[k])) {
      lo[0] = fminf(lo[0], X[k]); hi[0] = fmaxf(hi[0], X[k]);
      lo[1] = fminf(lo[1], Y[k]); hi[1] = fmaxf(hi[1], Y[k]);
      lo[2] = fminf(lo[2], Z[k]); hi[2] = fmaxf(hi[2], Z[k]);
    }
  }
  const bool any_here = win[0] || win[1] || win[2] || win[3];
  const unsigned long long any_wave = __ballot(any_here);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = wave_min(lo[a]);
    hi[a] = wave_max(hi[a]);
  }
  if (lane == 0u) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      s_box[wave][a] = lo[a];
      s_box[wave][3 + a] = hi[a];
    }
    s_any[wave] = any_wave != 0ull ? 1u : 0u;
  }
  if (t < LIGHT_WORDS) s_mask[t] = 0u;
  __syncthreads();
  if ((s_any[0] | s_any[1] | s_any[2] | s_any[3]) == 0u) {  // uniform: no winner in the tile
    if (t == 0u) L.tile_counts[tile] = 0u;
    return;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = fminf(fminf(s_box[0][a], s_box[1][a]), fminf(s_box[2][a], s_box[3][a]));
    hi[a] = fmaxf(fmaxf(s_box[0][3 + a], s_box[1][3 + a]), fmaxf(s_box[2][3 + a], s_box[3][3 + a]));
  }

  // ---- phase 2: the lights whose sphere meets the box
  for (uint32_t i = t; i < L.n_lights; i += 256u) {
    const float4 pr = reinterpret_cast<const float4*>(L.lights)[2u * i];  // position, radius
    const float gx = fmaxf(fmaxf(lo[0] - pr.x, pr.x - hi[0]), 0.0f);
    const float gy = fmaxf(fmaxf(lo[1] - pr.y, pr.y - hi[1]), 0.0f);
    const float gz = fmaxf(fmaxf(lo[2] - pr.z, pr.z - hi[2]), 0.0f);
    const float dbox2 = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
    if (dbox2 < pr.w * pr.w) atomicOr(&s_mask[i >> 5], 1u << (i & 31u));
  }
  __syncthreads();

  // ---- phase 3: the sun (C18), then the kept lights in index order (C19)
  float ar[4], ag[4], ab[4];
  const float sunw = L.sunlight_color[3];
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    ar[k] = ag[k] = ab[k] = 0.0f;
    if (!win[k]) continue;
    const float d = fmaf(nz[k], L.sunlight_direction[2], fmaf(ny[k], L.sunlight_direction[1], nx[k] * L.sunlight_direction[0]));
    bool shadowed = false;
    if (L.shadow.depth) {
      const Vec4 q = mat_vec(L.shadow.viewproj, X[k], Y[k], Z[k], 1.0f);
      shadowed = shadow_occluded(L.shadow, q.x, q.y, q.z, q.w);
    }
    const float light = shadowed ? 0.1f : fmaxf(d, 0.1f);
    if (AO) {
      const float ao = L.ao[at + k];
      ar[k] = fmaf(cr[k] * light, sunw, (cr[k] * L.ambient_color[0]) * ao);
      ag[k] = fmaf(cg[k] * light, sunw, (cg[k] * L.ambient_color[1]) * ao);
      ab[k] = fmaf(cb[k] * light, sunw, (cb[k] * L.ambient_color[2]) * ao);
    } else {
      ar[k] = fmaf(cr[k] * light, sunw, cr[k] * L.ambient_color[0]);
      ag[k] = fmaf(cg[k] * light, sunw, cg[k] * L.ambient_color[1]);
      ab[k] = fmaf(cb[k] * light, sunw, cb[k] * L.ambient_color[2]);
    }
  }
  uint32_t kept = 0;
  const uint32_t n_words = (L.n_lights + 31u) >> 5;
  for (uint32_t w = 0; w < n_words; w++) {
    uint32_t m = __builtin_amdgcn_readfirstlane(s_mask[w]);
    kept += __popc(m);
    while (m) {
      const uint32_t i = w * 32u + (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      const SvrPointLight& pl = L.lights[i];  // uniform address
      const float plx = pl.position[0], ply = pl.position[1], plz = pl.position[2];
      const float r2 = pl.radius * pl.radius;
      const float lr = pl.color[0], lg = pl.color[1], lb = pl.color[2], li = pl.intensity;
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        if (!win[k]) continue;
        const float vx = plx - X[k], vy = ply - Y[k], vz = plz - Z[k];
        const float d2 = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
        if (!(d2 < r2)) continue;
        const float ndl = fmaf(nz[k], vz, fmaf(ny[k], vy, nx[k] * vx));
        if (!(ndl > 0.0f)) continue;
        // `/` and sqrtf are correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
        const float tt = 1.0f - d2 / r2;
        const float kk = ((ndl / sqrtf(d2)) * ((tt * tt) / (d2 + 1.0f))) * li;
        ar[k] = fmaf(cr[k] * lr, kk, ar[k]);
        ag[k] = fmaf(cg[k] * lg, kk, ag[k]);
        ab[k] = fmaf(cb[k] * lb, kk, ab[k]);
      }
    }
  }
  if (t == 0u) L.tile_counts[tile] = kept;

  // ---- C20: encode and store the winners
  if (!any_here) return;
  if (FMT == SVR_COLOR_RGBA16F) {
    uint2* out = reinterpret_cast<uint2*>(L.color) + at;
    uint2 e[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) e[k] = encode16(ar[k], ag[k], ab[k]);
    if (win[0] && win[1] && win[2] && win[3] && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
      reinterpret_cast<uint4*>(out)[0] = make_uint4(e[0].x, e[0].y, e[1].x, e[1].y);
      reinterpret_cast<uint4*>(out)[1] = make_uint4(e[2].x, e[2].y, e[3].x, e[3].y);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (win[k]) out[k] = e[k];
    }
  } else {
    uint32_t* out = reinterpret_cast<uint32_t*>(L.color) + at;
    uint32_t e[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) e[k] = encode8(ar[k], ag[k], ab[k]);
    if (win[0] && win[1] && win[2] && win[3] && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
      *reinterpret_cast<uint4*>(out) = make_uint4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++)
        if (win[k]) out[k] = e[k];
    }
  }
}

void launch_light(const LightLaunch& L, int color_format, uint32_t tiles_y, hipStream_t s) {
  if (L.tiles_x == 0u || tiles_y == 0u) return;
  const dim3 grid(L.tiles_x, tiles_y), block(256);
  const bool f16 = color_format == SVR_COLOR_RGBA16F;
  if (L.ao) {
    if (f16) hipLaunchKernelGGL((light_kernel<SVR_COLOR_RGBA16F, true>), grid, block, 0, s, L);
    else hipLaunchKernelGGL((light_kernel<SVR_COLOR_RGBA8, true>), grid, block, 0, s, L);
  } else if (f16) hipLaunchKernelGGL((light_kernel<SVR_COLOR_RGBA16F, false>), grid, block, 0, s, L);
  else hipLaunchKernelGGL((light_kernel<SVR_COLOR_RGBA8, false>), grid, block, 0, s, L);
}

}  // namespace svr
