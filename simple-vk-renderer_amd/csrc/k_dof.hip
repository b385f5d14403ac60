// k_dof.hip — the depth of field pass (include/svr_dof.h): a signed blur radius per pixel from its depth, and a gather of
// 49 taps on a disc as wide as the largest radius near the pixel, over the RGBA16F colour target, in place.  Arithmetic:
// DESIGN.md C61-C66; ordering and the exactly-once argument: DESIGN.md §5 "Depth of field".
//
// Two kernels (launch_dof), both over 32 x 16 tiles of the scissor, which are 4 x 2 cells of 8 x 8 pixels:
//   dof_prepare_kernel   256 lanes.  A wave takes two cells side by side and a lane two pixels of a row: one 16-byte
//                        load where the pair is aligned and inside the scissor, one 16-byte store always (the prepared
//                        image's rows are padded to an even length).  It writes the prepared texels (the RGB halves
//                        after san, and the radius c) and reduces the largest |c| of each cell over the cell's 32 lanes.
//   dof_gather_kernel    512 lanes, a wave per cell and a lane per pixel.  A wave finds its cell's gather radius g first
//                        (the neighbour cells a lane each, reduced in the wave).  The prepared window, the tile and R
//                        texels around it (R: as far as the taps of the tile's cells reach, 0 for a tile in focus), is
//                        staged in LDS at clamped coordinates, so the array holds the edge-clamped image and no tap
//                        needs a test.  Rows are 72 texels apart: the four rows a 32-lane half reads with one 8-byte
//                        read per lane then lie on four different quarters of the 64 banks.  g is the cell's, so a
//                        tap's offset, its distance and whether it is skipped are the same for the whole wave: lane k
//                        works tap k out once (C64), and the loop reads offset and distance lane by lane into scalar
//                        registers and skips a zero offset on a uniform branch.  A cell with g < 0.5 skips the loop
//                        and copies its texels.
// Ordinary vector loads and stores only; nothing is handed between workgroups of one launch (the gather reads what the
// prepare's launch wrote, in stream order, and writes only its own pixels of the colour target).  Both kernels read the
// context's poison flag first: after an overflow they write nothing.
#include "svr_launch.h"
#include "svr_pixel.h"

#define SVR_DOF_TABLE __device__ const
#include "svr_dof_taps.h"

namespace svr {

namespace {

constexpr uint32_t GT_W = 32, GT_H = 16;                 // a tile of pixels
constexpr uint32_t CELL = 8;                             // C63
constexpr uint32_t WIN_W = GT_W + 2 * SVR_DOF_MAX_RADIUS, WIN_H = GT_H + 2 * SVR_DOF_MAX_RADIUS;  // the largest window
constexpr uint32_t WIN_PITCH = WIN_W + 8;                // texels: 144 dwords, 16 more than two bank rows
static_assert(WIN_W == 64, "the staging loop takes a window row per wave");

// C61: the signed radius of a pixel of depth d, as a half
__device__ __forceinline__ uint32_t dof_radius(const DofLaunch& A, float d) {
  const float iz = fmaf(d, A.inv_z_scale, A.inv_z_bias);
  float r = A.blur_scale * fmaf(A.neg_focus, iz, 1.0f);
  r = r == r ? r : 0.0f;
  r = r > A.neg_max_radius ? r : A.neg_max_radius;
  r = r < A.max_radius ? r : A.max_radius;
  return h16(r);
}

// C62: a prepared texel: san of the three RGB halves (exact: a half's san is a half), and c in the alpha half's place
__device__ __forceinline__ uint2 dof_prepared(uint2 texel, uint32_t c) {
  const Rgb in = decode_rgb(texel);
  return encode_rgb({san(in.r), san(in.g), san(in.b)}, make_uint2(0u, c << 16));
}

__device__ __forceinline__ float sat(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

}  // namespace

__global__ __launch_bounds__(256) void dof_prepare_kernel(DofLaunch A) {
  if (*A.poison) return;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  // (x, y): the lane's first pixel in the scissor; x is even
  const uint32_t x = blockIdx.x * GT_W + (wave & 1u) * 16u + 2u * (lane & 7u), y = blockIdx.y * GT_H + (wave >> 1) * CELL + (lane >> 3);
  const bool in_a = x < A.sw && y < A.sh, in_b = x + 1u < A.sw && y < A.sh;
  uint32_t m = 0u;  // the largest |c| of the lane's pixels, as half bits (their order is the values')
  if (in_a) {
    const size_t at = (size_t)(A.sy + y) * A.W + A.sx + x;
    const uint2* px = A.color + at;
    const float* dz = A.depth + at;
    uint2 ta, tb = make_uint2(0u, 0u);
    uint32_t ca, cb = 0u;
    if (in_b && aligned_to(px, 16u)) {
      const uint4 q = *reinterpret_cast<const uint4*>(px);
      ta = make_uint2(q.x, q.y);
      tb = make_uint2(q.z, q.w);
    } else {
      ta = px[0];
      if (in_b) tb = px[1];
    }
    ca = dof_radius(A, dz[0]);  // (a caller's depth target need not share the colour target's alignment)
    const uint2 pa = dof_prepared(ta, ca);
    uint2 pb = make_uint2(0u, 0u);  // the padding of an odd row: never read
    m = ca & 0x7fffu;
    if (in_b) {
      cb = dof_radius(A, dz[1]);
      pb = dof_prepared(tb, cb);
      m = max(m, cb & 0x7fffu);
    }
    // x is even and the pitch is even: the pair is aligned, and x + 1 < pitch
    *reinterpret_cast<uint4*>(A.prep + (size_t)y * A.pitch + x) = make_uint4(pa.x, pa.y, pb.x, pb.y);
  }
  // C63: M(cell) over the cell's 32 lanes: lane bits 0, 1 (its four pairs of a row) and 3, 4, 5 (its rows); bit 2 tells
  // the wave's two cells apart.  Every lane of the wave is here.
  m = max(m, (uint32_t)__shfl_xor((int)m, 1));
  m = max(m, (uint32_t)__shfl_xor((int)m, 2));
  m = max(m, (uint32_t)__shfl_xor((int)m, 8));
  m = max(m, (uint32_t)__shfl_xor((int)m, 16));
  m = max(m, (uint32_t)__shfl_xor((int)m, 32));
  if ((lane & ~4u) == 0u) {
    const uint32_t cx = blockIdx.x * (GT_W / CELL) + (wave & 1u) * 2u + (lane >> 2), cy = blockIdx.y * (GT_H / CELL) + (wave >> 1);
    if (cx < A.cw && cy < A.ch) A.cells[(size_t)cy * A.cw + cx] = half_bits_to_float(m);
  }
}

__global__ __launch_bounds__(512) void dof_gather_kernel(DofLaunch A) {
  if (*A.poison) return;
  __shared__ uint2 s_win[WIN_H * WIN_PITCH];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
  // ---- a wave per cell.  C63: g, the largest M within Rc cells (a cell outside the grid: 0)
  __shared__ float s_g[GT_W / CELL * (GT_H / CELL)];
  const uint32_t cx = blockIdx.x * (GT_W / CELL) + (wave & 3u), cy = blockIdx.y * (GT_H / CELL) + (wave >> 2);
  const bool in_grid = cx < A.cw && cy < A.ch;
  float g = 0.0f;
  if (in_grid) {
    // the 9 or 25 cells at once, a lane each (one after the other they are a chain of dependent loads, and a tile in
    // focus does little else), then the largest over the wave's first 32 lanes; every lane of the wave is here
    const uint32_t n = 2u * A.Rc + 1u;
    if (lane < n * n) {
      const uint32_t j = lane / n, i = lane - j * n;
      g = A.cells[(size_t)clamp_to((int)(cy + j) - (int)A.Rc, A.ch) * A.cw + clamp_to((int)(cx + i) - (int)A.Rc, A.cw)];
    }
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
      const float v = __shfl_xor(g, m);
      g = v > g ? v : g;
    }
    g = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, g)));
  }
  if (lane == 0u) s_g[wave] = g;
  __syncthreads();
  // ---- the window: the tile and R texels around it, read at clamped coordinates; a wave takes a row at a time.  R is
  // the farthest any tap of the tile's cells reaches, rint of their largest g (|u| <= 1): 0 for a tile in focus, at most
  // ceil(max_radius) (C61)
  float gm = s_g[0];
#pragma unroll
  for (uint32_t i = 1; i < GT_W / CELL * (GT_H / CELL); i++) gm = s_g[i] > gm ? s_g[i] : gm;
  int R = __builtin_amdgcn_readfirstlane((int)rintf(gm));
  R = R < 0 ? 0 : (R > SVR_DOF_MAX_RADIUS ? SVR_DOF_MAX_RADIUS : R);  // (never binds: |c| <= ceil(max_radius); the window is this large)
  {
    const int ox = (int)(blockIdx.x * GT_W) - R, oy = (int)(blockIdx.y * GT_H) - R;
    const uint32_t ww = GT_W + 2u * (uint32_t)R, wh = GT_H + 2u * (uint32_t)R;
    if (lane < ww) {
      const uint32_t gx = clamp_to(ox + (int)lane, A.sw);
      for (uint32_t wy = wave; wy < wh; wy += 8u) s_win[wy * WIN_PITCH + lane] = A.prep[(size_t)clamp_to(oy + (int)wy, A.sh) * A.pitch + gx];
    }
  }
  __syncthreads();
  if (!in_grid) return;  // the whole wave, behind the barriers
  const uint32_t lx = lane & 7u, ly = lane >> 3;
  const uint32_t x = cx * CELL + lx, y = cy * CELL + ly;
  const int at_w = (int)(((wave >> 2) * CELL + ly + (uint32_t)R) * WIN_PITCH + (wave & 3u) * CELL + lx + (uint32_t)R);
  const uint2 own = s_win[at_w];
  Rgb out = decode_rgb(own);
  if (g >= 0.5f) {
    // C64: lane k works tap k out, once for the cell (|dx|, |dy| <= rint(g) <= R: inside the window)
    const uint32_t kk = lane < (uint32_t)SVR_DOF_TAPS ? lane : 0u;
    const int dx = (int)rintf(SVR_DOF_TAP[kk][0] * g), dy = (int)rintf(SVR_DOF_TAP[kk][1] * g);
    const int my_off = dy * (int)WIN_PITCH + dx;  // 0 only where dx == dy == 0
    // sqrtf and `/` are correctly rounded: the file is built with -fhip-fp32-correctly-rounded-divide-sqrt
    const int my_dist = __builtin_bit_cast(int, sqrtf((float)(dx * dx + dy * dy)));
    const float cp = half_bits_to_float(own.y >> 16), acp = fabsf(cp);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, W = 0.0f;
    for (int k = 0; k < SVR_DOF_TAPS; k++) {
      const int off = __builtin_amdgcn_readlane(my_off, k);
      if (k != 0 && off == 0) continue;
      const float dist = __builtin_bit_cast(float, __builtin_amdgcn_readlane(my_dist, k));
      const uint2 tap = s_win[at_w + off];
      // C65
      const float ck = half_bits_to_float(tap.y >> 16), ack = fabsf(ck);
      const float e = ck > cp ? (ack < acp ? ack : acp) : ack;
      const float e2 = e * e;
      const float w = sat((e - dist) + 1.0f) / (e2 > 1.0f ? e2 : 1.0f);
      // C66
      const Rgb I = decode_rgb(tap);
      ar = fmaf(w, I.r, ar);
      ag = fmaf(w, I.g, ag);
      ab = fmaf(w, I.b, ab);
      W = W + w;
    }
    out = {san(ar / W), san(ag / W), san(ab / W)};
  }
  if (x < A.sw && y < A.sh) {
    uint2* px = A.color + (size_t)(A.sy + y) * A.W + A.sx + x;
    *px = encode_rgb(out, *px);  // the alpha half as it was
  }
}

void launch_dof(const DofLaunch& A, hipStream_t s) {
  if (A.sw == 0u || A.sh == 0u) return;
  const dim3 grid((A.sw + GT_W - 1u) / GT_W, (A.sh + GT_H - 1u) / GT_H);
  hipLaunchKernelGGL(dof_prepare_kernel, grid, dim3(256), 0, s, A);
  hipLaunchKernelGGL(dof_gather_kernel, grid, dim3(512), 0, s, A);
}

}  // namespace svr
