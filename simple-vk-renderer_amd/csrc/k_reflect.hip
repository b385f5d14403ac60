// k_reflect.hip — the reflection pass (include/svr_reflect.h): one screen-space ray per opaque pixel, marched through the
// depth target in equal world-space steps and refined by bisection, and the colour found at the hit blended over the
// RGBA16F colour target, in place.  Arithmetic: DESIGN.md C73-C79; ordering and the exactly-once argument: DESIGN.md §5
// "Reflection pass".
//
// Two kernels (launch_reflect):
//   reflect_trace_kernel       one lane per scissor pixel, a wave on an 8 x 8 cell, four cells side by side per workgroup:
//                              neighbouring rays walk neighbouring depth texels.  A lane sets its ray up once (h0, dh,
//                              the dither and the Fresnel term), then walks C75's loop: three fma, a reciprocal, two fma
//                              and two floors, one depth texel, one fma and one product per sample.  It reads the colour
//                              target only at the hit and writes only its 16-byte trace texel; the wave's lane 0 stores
//                              whether any texel of the cell is not 0, one ballot.
//   reflect_resolve_kernel<R>  one workgroup of 256 lanes per 32 x 16 tile of the scissor.  A tile none of whose cells (with
//                              R, those its taps reach too) holds a texel other than 0 takes san of the target's own
//                              texels and stores only those san changes; it reads neither trace texel nor depth.  With R
//                              the 34 x 18 window of trace texels and 1 / z is staged in LDS at clamped coordinates, so
//                              the arrays hold the edge-clamped image and no tap needs a test.  A lane takes two pixels:
//                              one 16-byte load and store where the pair is aligned and inside the scissor.
// The LDS pitch.  A tap is one 16-byte read per lane, served in groups of 16 lanes over 16 slots of 16 bytes, slot = texel
// index mod 16 (k_motion.hip has the groups).  A lane's pixels are two texels apart and a group takes eight lanes from
// each of two rows, so within a row the slots are eight of one parity; an odd pitch puts the other row's on the other
// parity.  35 is the first odd pitch that holds the window.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch (the resolve reads what the
// trace's launch wrote, in stream order, and writes only its own pixels of the colour target; the trace writes no colour,
// so every hit reads the target as it was before the pass).  Every address is formed from lane and block indices,
// clamped integers, or a sample's pixel after it passed the scissor test as floats (the extents are below 2^24: exact).
// Both kernels read the context's poison flag first: after an overflow they write nothing.
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

namespace svr {

namespace {

constexpr uint32_t WINNER_BITS = 0x3F800000u;  // the albedo texel's w of an opaque winner (include/svr_attributes.h)
constexpr uint32_t CELL = 8;
constexpr uint32_t RT_W = 32, RT_H = 16;           // the resolve's tile of pixels
constexpr uint32_t RS_W = RT_W + 2, RS_H = RT_H + 2;  // ... and the window staged for it
constexpr uint32_t RS_PITCH = RS_W + 1;            // texels: odd (see above)
static_assert(RS_PITCH % 2 == 1, "the bank rule of a 16-byte read, two texels per lane");

// NaN included: 0
__device__ __forceinline__ float sat(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// C56's hash, of the pixel (k_fog.hip hashes its block with the same function)
__device__ __forceinline__ uint32_t dither_hash(uint32_t x, uint32_t y, uint32_t frame) {
  uint32_t h = (x * 0x9E3779B1u) ^ (y * 0x85EBCA77u) ^ (frame * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

struct Ray {
  float hx, hy, hw, dx, dy, dw;  // h0 and dh: x, y and w
};

// C75: the sample at t.  0: outside; 1: inside and in front; 2: behind and too deep to be a hit; 3: a hit.  (fx, fy): the
// sample's pixel in the target, set unless the sample is outside
enum : int { S_OUTSIDE = 0, S_FRONT = 1, S_PASSED = 2, S_HIT = 3 };
__device__ __forceinline__ int sample_at(const ReflectLaunch& A, const Ray& r, float t, uint32_t& fx, uint32_t& fy) {
  const float hx = fmaf(r.dx, t, r.hx), hy = fmaf(r.dy, t, r.hy), hw = fmaf(r.dw, t, r.hw);
  if (!(hw > 0.0f)) return S_OUTSIDE;
  const float rw = rcp_ieee(hw);
  const float px = floorf(fmaf(hx * rw, A.half_w, A.half_w)), py = floorf(fmaf(hy * rw, A.half_h, A.half_h));
  // (a NaN fails; a passing floor is an index inside the scissor)
  if (!(px >= A.x_lo && px < A.x_hi && py >= A.y_lo && py < A.y_hi)) return S_OUTSIDE;
  fx = (uint32_t)px;
  fy = (uint32_t)py;
  const float q = hw * fmaf(A.depth[(size_t)fy * A.W + fx], A.inv_z_scale, A.inv_z_bias);
  return q >= 1.0f ? (q <= A.q_max ? S_HIT : S_PASSED) : S_FRONT;
}

// C73-C77 for the pixel (px, py) of the target: its trace texel
__device__ __forceinline__ float4 trace_pixel(const ReflectLaunch& A, uint32_t px, uint32_t py) {
  const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const size_t at = (size_t)py * A.W + px;
  // ---- C73
  const float z = A.depth[at];
  const float aw = reinterpret_cast<const float*>(A.albedo + at)[3];
  const float4 n = A.normal[at];
  const float nn = fmaf(n.z, n.z, fmaf(n.y, n.y, n.x * n.x));
  if (f2u(aw) != WINNER_BITS || f2u(z) == 0u || !(nn > 0.0f)) return none;
  // ---- C74.  sqrtf is correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
  const Vec4 h = unproject(A.inv_viewproj, pixel_ndc(px, A.two_over_w), pixel_ndc(py, A.two_over_h), z);
  const float rw = rcp_ieee(h.w);
  const float wx = h.x * rw, wy = h.y * rw, wz = h.z * rw;
  const float ux = wx - A.cam[0], uy = wy - A.cam[1], uz = wz - A.cam[2];
  const float vv = fmaf(uz, uz, fmaf(uy, uy, ux * ux));
  if (!(vv > 0.0f && vv < __builtin_inff())) return none;
  const float rn = rcp_ieee(sqrtf(nn)), rv = rcp_ieee(sqrtf(vv));
  const float nx = n.x * rn, ny = n.y * rn, nz = n.z * rn;
  const float vx = ux * rv, vy = uy * rv, vz = uz * rv;
  const float d = fmaf(nz, vz, fmaf(ny, vy, nx * vx));
  const float m2d = -2.0f * d;
  const float rx = fmaf(m2d, nx, vx), ry = fmaf(m2d, ny, vy), rz = fmaf(m2d, nz, vz);
  const Vec4 h0 = mat_vec(A.viewproj, wx, wy, wz, 1.0f), dh = mat_vec(A.viewproj, rx, ry, rz, 0.0f);  // (the z rows are not used)
  const Ray ray = {h0.x, h0.y, h0.w, dh.x, dh.y, dh.w};
  // ---- C75
  const float o = (float)(dither_hash(px, py, A.frame) >> 24) * 0x1p-8f;
  uint32_t fx = 0u, fy = 0u;
  float t_hit = 0.0f;
  bool found = false;
  for (uint32_t i = 1; i <= A.steps; i++) {
    const float t = ((float)i + o) * A.delta;
    const int s = sample_at(A, ray, t, fx, fy);
    if (s == S_OUTSIDE) break;
    if (s == S_HIT) {
      found = true;
      t_hit = t;
      break;
    }
  }
  if (!found) return none;
  // ---- C76
  float lo = t_hit - A.delta, hi = t_hit;
  for (uint32_t j = 0; j < A.refine; j++) {
    const float mid = 0.5f * (lo + hi);
    uint32_t mx = 0u, my = 0u;
    if (sample_at(A, ray, mid, mx, my) >= S_PASSED) {
      hi = mid;
      fx = mx;
      fy = my;
    } else {
      lo = mid;
    }
  }
  t_hit = hi;
  // ---- C77
  const float m = 1.0f - sat(-d), m2 = m * m;
  const float F = fmaf(A.one_minus_f0, (m2 * m2) * m, A.f0);
  const float fd = sat(fmaf(-(t_hit * A.rmax), A.distance_fade, 1.0f));
  float fe = 1.0f;
  if (A.inv_edge > 0.0f) {
    const uint32_t ex = min(fx - A.sx, A.sx + A.sw - 1u - fx), ey = min(fy - A.sy, A.sy + A.sh - 1u - fy);
    fe = sat(((float)min(ex, ey) + 0.5f) * A.inv_edge);
  }
  const float k = sat(((A.intensity * F) * fd) * fe);
  const Rgb c = decode_rgb(A.color[(size_t)fy * A.W + fx]);
  return make_float4(k * san(c.r), k * san(c.g), k * san(c.b), k);
}

// C79 for one pixel
__device__ __forceinline__ uint2 composite(uint2 texel, float4 acc, float ws) {
  const float rws = rcp_ieee(ws), kb = acc.w * rws;
  const Rgb in = decode_rgb(texel);
  const float r = san(in.r), g = san(in.g), b = san(in.b);
  return encode_rgb({san(fmaf(acc.x, rws, fmaf(-kb, r, r))), san(fmaf(acc.y, rws, fmaf(-kb, g, g))), san(fmaf(acc.z, rws, fmaf(-kb, b, b)))}, texel);
}

// C78 with the 3 x 3 resolve, then C79: the pixel at (lx, ly) of the staged window
__device__ __forceinline__ uint2 resolve_pixel(const ReflectLaunch& A, uint2 texel, const float4* s_tr, const float* s_iz, uint32_t lx, uint32_t ly) {
  const uint32_t c = ly * RS_PITCH + lx;
  const float izc = s_iz[c], tol = A.depth_tolerance * izc;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float ws = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const uint32_t j = (uint32_t)((int)c + dy * (int)RS_PITCH + dx);
      if ((dx == 0 && dy == 0) || fabsf(s_iz[j] - izc) <= tol) {
        const float4 v = s_tr[j];
        acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w;
        ws = ws + 1.0f;
      }
    }
  return composite(texel, acc, ws);
}

// san of a texel's RGB halves, the alpha half as it was
__device__ __forceinline__ uint2 san_texel(uint2 old) {
  const Rgb in = decode_rgb(old);
  return encode_rgb({san(in.r), san(in.g), san(in.b)}, old);
}

}  // namespace

__global__ __launch_bounds__(256) void reflect_trace_kernel(ReflectLaunch A) {
  if (*A.poison) return;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t cx = blockIdx.x * 4u + wave, cy = blockIdx.y;
  const uint32_t x = cx * CELL + (lane & 7u), y = cy * CELL + (lane >> 3);
  bool lit = false;
  if (x < A.sw && y < A.sh) {
    const float4 texel = trace_pixel(A, A.sx + x, A.sy + y);
    A.trace[(size_t)y * A.sw + x] = texel;
    lit = texel.w != 0.0f;  // (k == 0: the whole texel is 0)
  }
  // every lane of the wave is here
  const bool any = __builtin_amdgcn_ballot_w64(lit) != 0ull;
  if (lane == 0u && cx < A.cw && cy < A.ch) A.cells[(size_t)cy * A.cw + cx] = any ? 1u : 0u;
}

template <bool RESOLVE>
__global__ __launch_bounds__(256) void reflect_resolve_kernel(ReflectLaunch A) {
  if (*A.poison) return;
  __shared__ float4 s_tr[RESOLVE ? RS_H * RS_PITCH : 1];
  __shared__ float s_iz[RESOLVE ? RS_H * RS_PITCH : 1];
  const uint32_t t = threadIdx.x;
  const uint32_t x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H;  // inside the scissor
  constexpr int RIM = RESOLVE ? 1 : 0;
  // ---- the cells the tile's taps reach, at clamped coordinates: at most 6 x 4, a lane each
  int lit = 0;
  {
    const uint32_t ca = clamp_to((int)x0 - RIM, A.sw) / CELL, cb = clamp_to((int)(x0 + RT_W) - 1 + RIM, A.sw) / CELL;
    const uint32_t ra = clamp_to((int)y0 - RIM, A.sh) / CELL, rb = clamp_to((int)(y0 + RT_H) - 1 + RIM, A.sh) / CELL;
    const uint32_t n = cb - ca + 1u, m = rb - ra + 1u;
    if (t < n * m) {
      const uint32_t j = t / n, i = t - j * n;
      lit = (int)A.cells[(size_t)(ra + j) * A.cw + ca + i];
    }
  }
  lit = __syncthreads_or(lit);  // the same for every lane of the workgroup
  const uint32_t x = x0 + 2u * (t & 15u), y = y0 + (t >> 4);
  const bool inside = x < A.sw && y < A.sh, two = x + 1u < A.sw;
  const size_t at = (size_t)(A.sy + y) * A.W + A.sx + x;
  uint2* px = A.color + at;
  if (!lit) {
    // ---- every trace texel a pixel of the tile could take is 0: C79 leaves san(input), and a texel san does not change is
    // not stored again
    if (!inside) return;
    const uint2 a = px[0], sa = san_texel(a);
    if (sa.x != a.x || sa.y != a.y) px[0] = sa;
    if (two) {
      const uint2 b = px[1], sb = san_texel(b);
      if (sb.x != b.x || sb.y != b.y) px[1] = sb;
    }
    return;
  }
  if (RESOLVE) {
    // ---- the window: the tile and one texel around it, read at clamped coordinates
    for (uint32_t i = t; i < RS_W * RS_H; i += 256u) {
      const uint32_t r = i / RS_W, c = i - r * RS_W;
      const uint32_t gx = clamp_to((int)(x0 + c) - 1, A.sw), gy = clamp_to((int)(y0 + r) - 1, A.sh);
      s_tr[r * RS_PITCH + c] = A.trace[(size_t)gy * A.sw + gx];
      s_iz[r * RS_PITCH + c] = fmaf(A.depth[(size_t)(A.sy + gy) * A.W + A.sx + gx], A.inv_z_scale, A.inv_z_bias);
    }
    __syncthreads();
  }
  if (!inside) return;
  const uint32_t lx = x - x0 + 1u, ly = y - y0 + 1u;
  const float4* tr = A.trace + (size_t)y * A.sw + x;
  if (two && aligned_to(px, 16u)) {
    const uint4 q = *reinterpret_cast<const uint4*>(px);
    uint2 a, b;
    if (RESOLVE) {
      a = resolve_pixel(A, make_uint2(q.x, q.y), s_tr, s_iz, lx, ly);
      b = resolve_pixel(A, make_uint2(q.z, q.w), s_tr, s_iz, lx + 1u, ly);
    } else {  // C78 with one tap
      a = composite(make_uint2(q.x, q.y), tr[0], 1.0f);
      b = composite(make_uint2(q.z, q.w), tr[1], 1.0f);
    }
    *reinterpret_cast<uint4*>(px) = make_uint4(a.x, a.y, b.x, b.y);
  } else {
    px[0] = RESOLVE ? resolve_pixel(A, px[0], s_tr, s_iz, lx, ly) : composite(px[0], tr[0], 1.0f);
    if (two) px[1] = RESOLVE ? resolve_pixel(A, px[1], s_tr, s_iz, lx + 1u, ly) : composite(px[1], tr[1], 1.0f);
  }
}

void launch_reflect(const ReflectLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 block(256);
  hipLaunchKernelGGL(reflect_trace_kernel, dim3((A.sw + 4u * CELL - 1u) / (4u * CELL), (A.sh + CELL - 1u) / CELL), block, 0, s, A);
  const dim3 tiles((A.sw + RT_W - 1u) / RT_W, (A.sh + RT_H - 1u) / RT_H);
  if (A.resolve)
    hipLaunchKernelGGL(reflect_resolve_kernel<true>, tiles, block, 0, s, A);
  else
    hipLaunchKernelGGL(reflect_resolve_kernel<false>, tiles, block, 0, s, A);
}

}  // namespace svr
