// k_motion.hip — the camera motion blur pass (include/svr_motion.h): a velocity per pixel from its depth and the
// reprojection matrix, and a gather of 16 or 32 taps along the dominant velocity near the pixel, over the RGBA16F colour
// target, in place.  Arithmetic: DESIGN.md C67-C72; ordering and the exactly-once argument: DESIGN.md §5 "Motion blur".
//
// Two kernels (launch_motion), both over 32 x 16 tiles of the scissor, which are 4 x 2 cells of 8 x 8 pixels, 512 lanes, a
// wave per cell and a lane per pixel:
//   motion_prepare_kernel  writes the prepared texels, 16 bytes each: the RGB halves after san, the two velocity halves
//                          and the depth's bits, one 16-byte store per lane.  The cell's largest key (C69) is a 64-bit
//                          maximum over the wave, six exchanges; lane 0 stores it.  Only this kernel knows where a velocity
//                          comes from.
//   motion_gather_kernel   A wave finds its cell's G first (the neighbour cells a lane each, reduced in the wave).  The
//                          prepared window, the tile and R texels around it (R: as far as the taps of the tile's cells
//                          reach), is staged in LDS at clamped coordinates, so the array holds the
//                          edge-clamped image and no tap needs a test.  G is the cell's, so a tap's offset, its distance
//                          and whether it is skipped are the same for the whole wave: lane k works tap k out once (C70),
//                          and the loop reads offset and distance lane by lane into scalar registers and skips a zero
//                          offset on a uniform branch.  A cell with L2 < 0.25 skips the loop and copies its texels; a
//                          tile of eight such cells stages nothing: it takes san of the target's own texels and stores
//                          only those san changes.
// The LDS pitch.  A tap is one 16-byte read per lane (ds_read_b128), which the LDS serves in four groups of 16 lanes,
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same plus 32, each over the 64 banks as 16 slots of 16 bytes, slot =
// texel index mod 16.  With lane = 8 row + column a group reads columns 0-3 of rows 0 and 3 and columns 4-7 of rows 1 and
// 2 (or the other halves); with rows P texels apart the four pieces start at slots 0, P + 4, 2 P + 4 and 3 P.  P = 8 mod
// 16 puts them at 0, 12, 4 and 8 (and 4, 8, 0, 12 for the other group): sixteen different slots, whatever the tap's
// offset adds to all of them.  P = 72 is the first such pitch that holds the widest window, 64 texels.  The staging
// writes a row of consecutive texels per wave.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch (the gather reads what the
// prepare's launch wrote, in stream order, and writes only its own pixels of the colour target).  Every address is formed
// from lane and block indices and clamped integers; a depth, whatever its bits, only ever enters arithmetic.  Both kernels
// read the context's poison flag first: after an overflow they write nothing.
#include "svr_launch.h"
#include "svr_pixel.h"
#include "svr_screen_math.h"

namespace svr {

namespace {

constexpr uint32_t GT_W = 32, GT_H = 16;                 // a tile of pixels
constexpr uint32_t CELL = 8;                             // C69
constexpr uint32_t CELLS = GT_W / CELL * (GT_H / CELL);  // of a tile: its waves
constexpr uint32_t WIN_W = GT_W + 2 * SVR_MOTION_MAX_BLUR, WIN_H = GT_H + 2 * SVR_MOTION_MAX_BLUR;  // the largest window
constexpr uint32_t WIN_PITCH = WIN_W + 8;                // texels: 8 mod 16 (see above)
static_assert(WIN_W == 64, "the staging loop takes a window row per wave");
static_assert(WIN_PITCH % 16 == 8, "the bank rule of a 16-byte read");

// x > 0 ? (x < 1 ? x : 1) : 0 for an x that is no NaN (C71's is a sum of finite values): one clamp
__device__ __forceinline__ float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < __builtin_inff(); }  // (a NaN fails)

// C67: the velocity of pixel (px, py) of the target with depth z, as two halves (x low)
__device__ __forceinline__ uint32_t motion_velocity(const MotionLaunch& A, uint32_t px, uint32_t py, float z) {
  const Vec4 q = mat_vec(A.reproject, pixel_ndc(px, A.two_over_w), pixel_ndc(py, A.two_over_h), z, 1.0f);  // (q.z is not used)
  const float r = rcp_ieee(q.w);
  const float hx = fmaf(q.x * r, A.half_w, A.half_w), hy = fmaf(q.y * r, A.half_h, A.half_h);
  float vx = (((float)px + 0.5f) - hx) * A.half_shutter, vy = (((float)py + 0.5f) - hy) * A.half_shutter;
  if (!(q.w > 0.0f) || !is_finite(vx) || !is_finite(vy)) vx = vy = 0.0f;
  // sqrtf and `/` are correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
  const float l = sqrtf(fmaf(vy, vy, vx * vx));
  if (l > A.max_blur) {
    const float k = A.max_blur / l;
    vx *= k;
    vy *= k;
  }
  return h16(vx) | (h16(vy) << 16);
}

// C69: a texel's key from its velocity halves
__device__ __forceinline__ unsigned long long motion_key(uint32_t v) {
  const float vx = half_bits_to_float(v & 0xffffu), vy = half_bits_to_float(v >> 16);
  const float len2 = fmaf(vy, vy, vx * vx);
  return ((unsigned long long)__builtin_bit_cast(uint32_t, len2) << 32) | ((v & 0xffffu) << 16) | (v >> 16);
}

// the largest key of the wave's first `lanes` lanes (a power of two), in all of them
template <int lanes>
__device__ __forceinline__ unsigned long long wave_max(unsigned long long m) {
#pragma unroll
  for (int s = 1; s < lanes; s <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)m, s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), s);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    m = o > m ? o : m;
  }
  return m;
}

}  // namespace

__global__ __launch_bounds__(512) void motion_prepare_kernel(MotionLaunch A) {
  if (*A.poison) return;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t cx = blockIdx.x * (GT_W / CELL) + (wave & 3u), cy = blockIdx.y * (GT_H / CELL) + (wave >> 2);
  const uint32_t x = cx * CELL + (lane & 7u), y = cy * CELL + (lane >> 3);
  unsigned long long m = 0ull;  // a pixel outside the scissor: the smallest key
  if (x < A.sw && y < A.sh) {
    const size_t at = (size_t)(A.sy + y) * A.W + A.sx + x;
    const uint2 texel = A.color[at];
    const float z = A.depth[at];
    const uint32_t v = motion_velocity(A, A.sx + x, A.sy + y, z);
    // C68: san of a half is a half, so the encoding is exact; the alpha half's place holds nothing
    const Rgb in = decode_rgb(texel);
    const uint2 c = encode_rgb({san(in.r), san(in.g), san(in.b)}, make_uint2(0u, 0u));
    A.prep[(size_t)y * A.sw + x] = make_uint4(c.x, c.y, v, __builtin_bit_cast(uint32_t, z));
    m = motion_key(v);
  }
  // C69: M(cell); every lane of the wave is here
  m = wave_max<64>(m);
  if (lane == 0u && cx < A.cw && cy < A.ch) A.cells[(size_t)cy * A.cw + cx] = m;
}

__global__ __launch_bounds__(512) void motion_gather_kernel(MotionLaunch A) {
  if (*A.poison) return;
  __shared__ uint4 s_win[WIN_H * WIN_PITCH];
  __shared__ uint2 s_g[CELLS];  // G's low and high words
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
  // ---- a wave per cell.  C69: G, the largest M within Rc cells, clamped to the grid
  const uint32_t cx = blockIdx.x * (GT_W / CELL) + (wave & 3u), cy = blockIdx.y * (GT_H / CELL) + (wave >> 2);
  const bool in_grid = cx < A.cw && cy < A.ch;
  unsigned long long G = 0ull;
  if (in_grid) {
    // the 9 or 25 cells at once, a lane each, then the largest over the wave's first 32 lanes; every lane of the wave is here
    const uint32_t n = 2u * A.Rc + 1u;
    if (lane < n * n) {
      const uint32_t j = lane / n, i = lane - j * n;
      G = A.cells[(size_t)clamp_to((int)(cy + j) - (int)A.Rc, A.ch) * A.cw + clamp_to((int)(cx + i) - (int)A.Rc, A.cw)];
    }
    G = wave_max<32>(G);
  }
  const uint32_t g_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)G), g_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(G >> 32));
  if (lane == 0u) s_g[wave] = make_uint2(g_lo, g_hi);
  __syncthreads();
  const uint32_t lx = lane & 7u, ly = lane >> 3;
  const uint32_t x = cx * CELL + lx, y = cy * CELL + ly;
  // ---- a tile all of whose cells copy (C69: L2 < 0.25; L2 is not negative, so its bits order as its value) needs no
  // window and nothing of the prepared image: san of the target's own texel is the prepared colour, bit for bit, and a
  // texel san does not change is not stored again.  The same for every wave of the workgroup: none reaches the barrier below
  uint32_t lm = 0u;
#pragma unroll
  for (uint32_t i = 0; i < CELLS; i++) lm = max(lm, s_g[i].y);
  if (lm < 0x3e800000u) {  // the bits of 0.25f
    if (x < A.sw && y < A.sh) {  // (false for every lane of a wave outside the grid)
      uint2* px = A.color + (size_t)(A.sy + y) * A.W + A.sx + x;
      const uint2 old = *px;
      const Rgb in = decode_rgb(old);
      const uint2 now = encode_rgb({san(in.r), san(in.g), san(in.b)}, old);
      if (now.x != old.x || now.y != old.y) *px = now;
    }
    return;
  }
  // ---- the window: the tile and R texels around it, read at clamped coordinates; a wave takes a row at a time.  R is the
  // farthest any tap of the tile's cells reaches: |rint(g s)| <= ceil(|g|) for |s| < 1, at most ceil(max_blur) (C70).
  // |gx| and |gy| are halves without their sign bits, which order as their values
  uint32_t hm = 0u;
#pragma unroll
  for (uint32_t i = 0; i < CELLS; i++) {
    const uint32_t a = (s_g[i].x >> 16) & 0x7fffu, b = s_g[i].x & 0x7fffu;
    hm = max(hm, max(a, b));
  }
  int R = __builtin_amdgcn_readfirstlane((int)ceilf(half_bits_to_float(hm)));
  R = R < 0 ? 0 : (R > SVR_MOTION_MAX_BLUR ? SVR_MOTION_MAX_BLUR : R);  // (never binds: |v| <= ceil(max_blur); the window is this large)
  {
    const int ox = (int)(blockIdx.x * GT_W) - R, oy = (int)(blockIdx.y * GT_H) - R;
    const uint32_t ww = GT_W + 2u * (uint32_t)R, wh = GT_H + 2u * (uint32_t)R;
    if (lane < ww) {
      const uint32_t gx = clamp_to(ox + (int)lane, A.sw);
      for (uint32_t wy = wave; wy < wh; wy += CELLS) s_win[wy * WIN_PITCH + lane] = A.prep[(size_t)clamp_to(oy + (int)wy, A.sh) * A.sw + gx];
    }
  }
  __syncthreads();
  if (!in_grid) return;  // the whole wave, behind the barriers
  const int at_w = (int)(((wave >> 2) * CELL + ly + (uint32_t)R) * WIN_PITCH + (wave & 3u) * CELL + lx + (uint32_t)R);
  const uint4 own = s_win[at_w];
  Rgb out = decode_rgb(make_uint2(own.x, own.y));
  const float L2 = __builtin_bit_cast(float, g_hi);
  if (L2 >= 0.25f) {
    const float gx = half_bits_to_float(g_lo >> 16), gy = half_bits_to_float(g_lo & 0xffffu);
    // C70: lane k works tap k out, once for the cell: +s_0, -s_0, +s_1, ...; g s is exact (11 bits by 5), and
    // |dx|, |dy| <= ceil(|g|) <= R: inside the window
    const int n = L2 > 64.0f ? 32 : 16;
    const float rn = L2 > 64.0f ? 0.03125f : 0.0625f;  // 1 / n
    const float sa = (float)(lane | 1u) * rn, s = (lane & 1u) ? -sa : sa;  // (2 j + 1) / n, j = k >> 1: exact
    int dx = (int)rintf(gx * s), dy = (int)rintf(gy * s);
    dx = dx < -R ? -R : (dx > R ? R : dx);  // (never binds; no tap leaves the window whatever the cell image holds)
    dy = dy < -R ? -R : (dy > R ? R : dy);
    const int my_off = dy * (int)WIN_PITCH + dx;  // 0 only where dx == dy == 0 (|dx| < the pitch)
    const int my_dist = __builtin_bit_cast(int, sqrtf((float)(dx * dx + dy * dy)));
    // C71
    const float rgl = 1.0f / sqrtf(L2);
    const float zp = __builtin_bit_cast(float, own.w);
    const float ep = fabsf(fmaf(half_bits_to_float(own.z >> 16), gy, half_bits_to_float(own.z & 0xffffu) * gx)) * rgl;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, S = 0.0f;
    for (int k = 0; k < n; k++) {
      const int off = __builtin_amdgcn_readlane(my_off, k);
      if (off == 0) continue;  // weight 0, and it counts in n
      const float dist = __builtin_bit_cast(float, __builtin_amdgcn_readlane(my_dist, k));
      const uint4 tap = s_win[at_w + off];
      const float ek = fabsf(fmaf(half_bits_to_float(tap.z >> 16), gy, half_bits_to_float(tap.z & 0xffffu) * gx)) * rgl;
      const float e = __builtin_bit_cast(float, tap.w) < zp ? ep : ek;
      const float w = sat((e - dist) + 1.0f);
      // C72
      const Rgb I = decode_rgb(make_uint2(tap.x, tap.y));
      ar = fmaf(w, I.r, ar);
      ag = fmaf(w, I.g, ag);
      ab = fmaf(w, I.b, ab);
      S = S + w;
    }
    const float rest = (float)n - S;
    out = {san(fmaf(rest, out.r, ar) * rn), san(fmaf(rest, out.g, ag) * rn), san(fmaf(rest, out.b, ab) * rn)};
  }
  if (x < A.sw && y < A.sh) {
    uint2* px = A.color + (size_t)(A.sy + y) * A.W + A.sx + x;
    *px = encode_rgb(out, *px);  // the alpha half as it was
  }
}

void launch_motion(const MotionLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 grid((A.sw + GT_W - 1u) / GT_W, (A.sh + GT_H - 1u) / GT_H);
  hipLaunchKernelGGL(motion_prepare_kernel, grid, dim3(512), 0, s, A);
  hipLaunchKernelGGL(motion_gather_kernel, grid, dim3(512), 0, s, A);
}

}  // namespace svr
