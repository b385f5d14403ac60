// k_overlay.hip — the UI overlay pass (include/svr_overlay.h): 2D triangle lists with per-command clip boxes, blended in
// submission order over a UNORM8 image.  Arithmetic: DESIGN.md C43-C49; the design and its costs: DESIGN.md §5 "Overlay".
//
// Two kernels (launch_overlay), no sorting pass:
//   overlay_setup_kernel   a thread per triangle: finds its command by binary search over the commands' first-triangle
//                          numbers, fetches, snaps and orients the vertices, cuts the pixel box with the command's clip
//                          box and writes the record; counts the kept ones with one integer atomic per wave.
//   overlay_tile_kernel    a workgroup of 256 threads per 32 x 32 tile of the rectangle of tiles that the commands' clip
//                          boxes reach, a thread per four consecutive pixels of a row.
//                          It walks the commands in order, skipping those whose clip box misses the tile; of the others
//                          it tests OVERLAY_CHUNK record boxes at a time against the tile, a thread each, compacts the
//                          survivors in order (a ballot per wave, the four waves' counts through LDS) and stages their
//                          records in an LDS list of OVERLAY_KEPT.  When the list is full, and at the end, every thread
//                          walks it in order: a record is an LDS broadcast read, the three edge values step across the
//                          thread's pixels, and a covered pixel interpolates, samples, blends and quantises in registers.
//                          The destination is loaded before the first walk and stored after the last, by the threads
//                          that changed something; a workgroup that kept nothing touches no destination memory.
// Plain vector loads and stores, LDS and global integer atomics (the statistics) only.  Both kernels read the context's
// poison flag first and write nothing while it is raised.
#include "svr_launch.h"
#include "svr_pixel.h"

namespace svr {

// ---- capacities and the LDS budget (tests/test_overlay_gpu.py reads the two capacities from here)
constexpr uint32_t OVERLAY_CHUNK = 256;  // record boxes tested at a time: one per thread
constexpr uint32_t OVERLAY_KEPT = 128;   // records the LDS list holds before it is drained
constexpr uint32_t OVERLAY_TILE = 32;
// LDS: the list (OVERLAY_KEPT x 144 bytes = 18 KiB), the texture table (16 x 24 bytes) and two sets of the four waves'
// counts: eight workgroups would fit a compute unit's 160 KiB, more than its registers let run (profiles/overlay_kinfo.txt)
constexpr uint32_t OVERLAY_LDS_BYTES = OVERLAY_KEPT * OVERLAY_REC_WORDS * 4u + SVR_OVERLAY_MAX_TEXTURES * 24u + 2u * 4u * 4u;
static_assert(OVERLAY_LDS_BYTES <= 20u * 1024u, "the LDS budget of overlay_tile_kernel");
static_assert(OVERLAY_CHUNK == 256u && OVERLAY_REC_WORDS % 4u == 0u, "a box per thread; records move as 16-byte words");

namespace {

// ---- the record (OVERLAY_REC_WORDS words).  Edge k runs from vertex k+1 to vertex k+2 (C4, C44).
//   0      x0 | y0 << 16            the pixel box, cut to the clip box and the image; x1, y1 exclusive;
//   1      x1 | y1 << 16            a dead record has x1 = 0
//   2..7   dx0 dy0 dx1 dy1 dx2 dy2  int32, in 1/256 px
//   8..13  e0 e1 e2                 int64 (low word first): the edge value at pixel (0, 0)'s centre plus the top-left bias
//   14     inv                      1.0f / (float)area
//   15     texture | b1 << 8 | b2 << 9   b_k: edge k's bias is -1
//   16..21 u0 v0, u1-u0 v1-v0, u2-u0 v2-v0
//   22..33 the colour: chan(col0) [4], chan(col1) - chan(col0) [4], chan(col2) - chan(col0) [4]
//   34..35 unused
constexpr uint32_t R_BOX = 0, R_STEP = 2, R_EDGE = 8, R_INV = 14, R_TEX = 15, R_UV = 16, R_COL = 22;
constexpr float SNAP_MAX = 8388608.0f;  // 2^23, in 1/256 px

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void overlay_setup_kernel(OverlayLaunch A) {
  if (*A.poison) return;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  bool kept = false;
  if (t < A.n_tris) {
    // the command: the last one whose first triangle is <= t
    uint32_t lo = 0, hi = A.n_cmds;
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (A.cmds[mid].tri_first <= t) lo = mid; else hi = mid;
    }
    const OverlayCmdDev cmd = A.cmds[lo];
    const uint32_t first = cmd.idx_offset + 3u * (t - cmd.tri_first);
    int64_t X[3], Y[3];
    float u[3], v[3];
    uint32_t col[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const SvrOverlayVertex w = A.vertices[cmd.vtx_offset + A.indices[first + k]];
      const float x = (w.pos[0] - A.display_pos[0]) * A.scale[0], y = (w.pos[1] - A.display_pos[1]) * A.scale[1];
      ok = ok && finite_f(x) && finite_f(y);
      X[k] = (int64_t)fminf(fmaxf(rintf(x * 256.0f), -SNAP_MAX), SNAP_MAX);
      Y[k] = (int64_t)fminf(fmaxf(rintf(y * 256.0f), -SNAP_MAX), SNAP_MAX);
      u[k] = w.uv[0];
      v[k] = w.uv[1];
      col[k] = w.col;
    }
    int64_t area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (area < 0) {  // no culling: vertices 1 and 2 change places
      area = -area;
      const int64_t tx = X[1], ty = Y[1];
      X[1] = X[2]; Y[1] = Y[2]; X[2] = tx; Y[2] = ty;
      const float tu = u[1], tv = v[1];
      u[1] = u[2]; v[1] = v[2]; u[2] = tu; v[2] = tv;
      const uint32_t tc = col[1];
      col[1] = col[2]; col[2] = tc;
    }
    uint32_t* R = A.recs + (size_t)t * OVERLAY_REC_WORDS;
    uint2 box = make_uint2(0u, 0u);
    if (ok && area != 0) {
      const int64_t minx = min(X[0], min(X[1], X[2])), maxx = max(X[0], max(X[1], X[2]));
      const int64_t miny = min(Y[0], min(Y[1], Y[2])), maxy = max(Y[0], max(Y[1], Y[2]));
      // pixels whose centre 256 i + 128 lies in [min, max], cut to the clip box (which lies inside the image)
      const int64_t x0 = max((minx + 127) >> 8, (int64_t)cmd.x0), x1 = min(((maxx - 128) >> 8) + 1, (int64_t)cmd.x1);
      const int64_t y0 = max((miny + 127) >> 8, (int64_t)cmd.y0), y1 = min(((maxy - 128) >> 8) + 1, (int64_t)cmd.y1);
      if (x1 > x0 && y1 > y0) {
        kept = true;
        box = make_uint2((uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16));
        uint32_t bias_bits = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int a = (k + 1) % 3, b = (k + 2) % 3;
          const int64_t dx = X[b] - X[a], dy = Y[b] - Y[a];
          const int64_t bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
          const int64_t e = dx * (128 - Y[a]) - dy * (128 - X[a]) + bias;
          R[R_STEP + 2 * k] = (uint32_t)(int32_t)dx;
          R[R_STEP + 2 * k + 1] = (uint32_t)(int32_t)dy;
          R[R_EDGE + 2 * k] = (uint32_t)(uint64_t)e;
          R[R_EDGE + 2 * k + 1] = (uint32_t)((uint64_t)e >> 32);
          if (k > 0 && bias != 0) bias_bits |= 1u << (7 + k);
        }
        R[R_INV] = __float_as_uint(1.0f / (float)area);
        R[R_TEX] = cmd.texture | bias_bits;
        R[R_UV + 0] = __float_as_uint(u[0]);
        R[R_UV + 1] = __float_as_uint(v[0]);
        R[R_UV + 2] = __float_as_uint(u[1] - u[0]);
        R[R_UV + 3] = __float_as_uint(v[1] - v[0]);
        R[R_UV + 4] = __float_as_uint(u[2] - u[0]);
        R[R_UV + 5] = __float_as_uint(v[2] - v[0]);
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const float c0 = chan(col[0], c);
          R[R_COL + c] = __float_as_uint(c0);
          R[R_COL + 4 + c] = __float_as_uint(chan(col[1], c) - c0);
          R[R_COL + 8 + c] = __float_as_uint(chan(col[2], c) - c0);
        }
        R[34] = 0u;
        R[35] = 0u;
      }
    }
    R[R_BOX] = box.x;
    R[R_BOX + 1] = box.y;
    A.boxes[t] = box;
  }
  const unsigned long long m = __ballot(kept);
  if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(&A.stats[1], (uint32_t)__popcll(m));
}

// C47: one axis of the bilinear tap: the two texel indices, clamped to the edge, and the fraction
__device__ __forceinline__ void tap(float coord, uint32_t extent, uint32_t& i0, uint32_t& i1, float& frac) {
  const float s = coord * (float)extent - 0.5f, fs = floorf(s);
  frac = s - fs;
  const int i = (int)fminf(fmaxf(fs, -1.0f), (float)extent);  // a NaN ends at -1; the conversion is of a small integer
  i0 = clamp_to(i, extent);
  i1 = clamp_to(i + 1, extent);
}
__device__ __forceinline__ float filt(float a, float b, float c00, float c10, float c01, float c11) {
  const float top = fmaf(a, c10 - c00, c00), bot = fmaf(a, c11 - c01, c01);
  return fmaf(b, bot - top, top);
}

// A fragment in two steps, so that a thread's four pixels have their texel loads in flight together.
__device__ __forceinline__ float attr(const uint32_t* R, uint32_t at, uint32_t stride, float w1, float w2) {
  return fmaf(w2, __uint_as_float(R[at + 2 * stride]), fmaf(w1, __uint_as_float(R[at + stride]), __uint_as_float(R[at])));
}
struct Taps {
  uint32_t t00, t10, t01, t11;  // the four texels: words (RGBA8) or bytes (A8)
  float a, b;                   // the fractions
};
// C46, C47: the pixel's uv and its four texels.  Issued for uncovered pixels of the four too: whatever the uv, the taps
// are clamped into the texture, which a live record's table entry names.
__device__ __forceinline__ Taps fetch(float w1, float w2, const uint32_t* R, const SvrOverlayTexture& T) {
  const float u = attr(R, R_UV, 2, w1, w2), v = attr(R, R_UV + 1, 2, w1, w2);
  uint32_t i0, i1, j0, j1;
  Taps t;
  tap(u, T.width, i0, i1, t.a);
  tap(v, T.height, j0, j1, t.b);
  const size_t r0 = (size_t)j0 * T.width, r1 = (size_t)j1 * T.width;
  if (T.format == SVR_OVERLAY_TEX_A8) {
    const uint8_t* p = static_cast<const uint8_t*>(T.texels);
    t.t00 = p[r0 + i0]; t.t10 = p[r0 + i1]; t.t01 = p[r1 + i0]; t.t11 = p[r1 + i1];
  } else {
    const uint32_t* p = static_cast<const uint32_t*>(T.texels);
    t.t00 = p[r0 + i0]; t.t10 = p[r0 + i1]; t.t01 = p[r1 + i0]; t.t11 = p[r1 + i1];
  }
  return t;
}
// C46-C48: the fragment over the stored texel d
__device__ __forceinline__ uint32_t shade(uint32_t d, float w1, float w2, const uint32_t* R, const Taps& t, uint32_t format, bool bgr) {
  const float4 col = make_float4(attr(R, R_COL, 4, w1, w2), attr(R, R_COL + 1, 4, w1, w2), attr(R, R_COL + 2, 4, w1, w2), attr(R, R_COL + 3, 4, w1, w2));
  const float a = t.a, b = t.b;
  const uint32_t t00 = t.t00, t10 = t.t10, t01 = t.t01, t11 = t.t11;
  float4 tex;
  if (format == SVR_OVERLAY_TEX_A8) {
    tex = make_float4(1.0f, 1.0f, 1.0f, filt(a, b, chan(t00, 0), chan(t10, 0), chan(t01, 0), chan(t11, 0)));
  } else {
    tex = make_float4(filt(a, b, chan(t00, 0), chan(t10, 0), chan(t01, 0), chan(t11, 0)), filt(a, b, chan(t00, 1), chan(t10, 1), chan(t01, 1), chan(t11, 1)),
                      filt(a, b, chan(t00, 2), chan(t10, 2), chan(t01, 2), chan(t11, 2)), filt(a, b, chan(t00, 3), chan(t10, 3), chan(t01, 3), chan(t11, 3)));
  }
  const float sr = col.x * tex.x, sg = col.y * tex.y, sb = col.z * tex.z, sa = col.w * tex.w;
  const int rc = bgr ? 2 : 0, bc = bgr ? 0 : 2;
  const float ia = 1.0f - sa;
  const uint32_t r = un8(fmaf(sr, sa, chan(d, rc) * ia)), g = un8(fmaf(sg, sa, chan(d, 1) * ia)), bl = un8(fmaf(sb, sa, chan(d, bc) * ia));
  const uint32_t al = un8(fmaf(chan(d, 3), ia, sa));
  return (r << (8 * rc)) | (g << 8) | (bl << (8 * bc)) | (al << 24);
}

__global__ __launch_bounds__(256) void overlay_tile_kernel(OverlayLaunch A) {
  __shared__ __attribute__((aligned(16))) uint32_t s_rec[OVERLAY_KEPT * OVERLAY_REC_WORDS];
  __shared__ uint32_t s_cnt[2][4];
  __shared__ __attribute__((aligned(8))) uint32_t s_tex[SVR_OVERLAY_MAX_TEXTURES * 6];  // SvrOverlayTexture is six words
  if (*A.poison) return;
  // the texture table, once: read as broadcasts from here on (the first barrier below stands in front of the first walk)
  if (threadIdx.x < A.n_textures * 6u) s_tex[threadIdx.x] = reinterpret_cast<const uint32_t*>(A.textures)[threadIdx.x];
  // the grid is the tiles the commands' clip boxes reach (host-known), row by row
  const uint32_t TX0 = (A.tile_x0 + blockIdx.x % A.tiles_w) * OVERLAY_TILE, TY0 = (A.tile_y0 + blockIdx.x / A.tiles_w) * OVERLAY_TILE;
  const uint32_t TX1 = min(TX0 + OVERLAY_TILE, A.dw), TY1 = min(TY0 + OVERLAY_TILE, A.dh);
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t px = TX0 + (t & 7u) * 4u, py = TY0 + (t >> 3);
  const bool bgr = A.dst_fmt == SVR_SWAPCHAIN_B8G8R8A8;
  // one 16-byte access where the address allows: rows of a multiple of four texels from a 16-byte aligned base
  const bool wide = (A.dw & 3u) == 0u && aligned_to(A.dst, 16);
  uint32_t* const mine = A.dst + (size_t)py * A.dw + px;
  uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  bool loaded = false, touched = false, had = false;
  uint32_t n_list = 0, parity = 0;

  // every thread walks the list's first n records in order
  auto drain = [&](uint32_t n) {
    if (!loaded) {
      loaded = true;
      if (py < A.dh) {
        if (wide) {
          if (px < A.dw) {
            const uint4 q = *reinterpret_cast<const uint4*>(mine);
            d0 = q.x; d1 = q.y; d2 = q.z; d3 = q.w;
          }
        } else {
          if (px < A.dw) d0 = mine[0];
          if (px + 1u < A.dw) d1 = mine[1];
          if (px + 2u < A.dw) d2 = mine[2];
          if (px + 3u < A.dw) d3 = mine[3];
        }
      }
    }
    for (uint32_t r = 0; r < n; r++) {
      const uint32_t* R = s_rec + r * OVERLAY_REC_WORDS;
      const uint32_t b0 = R[R_BOX], b1 = R[R_BOX + 1];
      const uint32_t x0 = b0 & 0xffffu, y0 = b0 >> 16, x1 = b1 & 0xffffu, y1 = b1 >> 16;
      if (py < y0 || py >= y1 || px + 3u < x0 || px >= x1) continue;
      int64_t e[3], sx[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int64_t dx = (int32_t)R[R_STEP + 2 * k], dy = (int32_t)R[R_STEP + 2 * k + 1];
        const int64_t e0 = (int64_t)((uint64_t)R[R_EDGE + 2 * k] | ((uint64_t)R[R_EDGE + 2 * k + 1] << 32));
        sx[k] = -dy * 256;
        e[k] = e0 + (int64_t)py * (dx * 256) + (int64_t)px * sx[k];
      }
      const float inv = __uint_as_float(R[R_INV]);
      const int64_t u1 = (R[R_TEX] >> 8) & 1u, u2 = (R[R_TEX] >> 9) & 1u;  // what the bias took from edges 1 and 2
      bool in[4];
      float w1[4], w2[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t x = px + k;
        in[k] = x >= x0 && x < x1 && (e[0] | e[1] | e[2]) >= 0;
        w1[k] = (float)(e[1] + u1) * inv;
        w2[k] = (float)(e[2] + u2) * inv;
        e[0] += sx[0]; e[1] += sx[1]; e[2] += sx[2];
      }
      if (!(in[0] || in[1] || in[2] || in[3])) continue;
      const SvrOverlayTexture T = *reinterpret_cast<const SvrOverlayTexture*>(s_tex + (R[R_TEX] & 0xffu) * 6u);
      Taps taps[4];
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) taps[k] = fetch(w1[k], w2[k], R, T);  // sixteen loads in flight
#pragma unroll
      for (uint32_t k = 0; k < 4u; k++) {
        if (in[k]) {
          uint32_t& d = k == 0 ? d0 : (k == 1 ? d1 : (k == 2 ? d2 : d3));
          d = shade(d, w1[k], w2[k], R, taps[k], T.format, bgr);
          touched = true;
        }
      }
    }
  };

  for (uint32_t c = 0; c < A.n_cmds; c++) {
    const OverlayCmdDev& cmd = A.cmds[c];
    // the cut that matters: a command is a window, and most windows miss most tiles
    if (cmd.x1 <= (int32_t)TX0 || cmd.x0 >= (int32_t)TX1 || cmd.y1 <= (int32_t)TY0 || cmd.y0 >= (int32_t)TY1) continue;
    const uint32_t tri_first = cmd.tri_first, tri_count = cmd.tri_count;
    for (uint32_t base = 0; base < tri_count; base += OVERLAY_CHUNK) {
      const uint32_t i = base + t;
      bool hit = false;
      if (i < tri_count) {
        const uint2 b = A.boxes[tri_first + i];
        const uint32_t x0 = b.x & 0xffffu, y0 = b.x >> 16, x1 = b.y & 0xffffu, y1 = b.y >> 16;
        hit = x1 > x0 && x0 < TX1 && x1 > TX0 && y0 < TY1 && y1 > TY0;
      }
      const unsigned long long m = __ballot(hit);
      if (lane == 0u) s_cnt[parity][wave] = (uint32_t)__popcll(m);
      __syncthreads();
      const uint32_t c0 = s_cnt[parity][0], c1 = s_cnt[parity][1], c2 = s_cnt[parity][2], c3 = s_cnt[parity][3];
      parity ^= 1u;  // the next chunk's counts go to the other set: no second barrier
      const uint32_t total = c0 + c1 + c2 + c3;
      if (total == 0u) continue;
      had = true;
      const uint32_t pos = (wave > 0u ? c0 : 0u) + (wave > 1u ? c1 : 0u) + (wave > 2u ? c2 : 0u) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      uint32_t done = 0;
      while (done < total) {  // (total, done and n_list are the same in every thread)
        const uint32_t take = min(OVERLAY_KEPT - n_list, total - done);
        if (hit && pos >= done && pos < done + take) {
          const uint4* src = reinterpret_cast<const uint4*>(A.recs + (size_t)(tri_first + i) * OVERLAY_REC_WORDS);
          uint4* dst = reinterpret_cast<uint4*>(s_rec + (n_list + pos - done) * OVERLAY_REC_WORDS);
#pragma unroll
          for (uint32_t q = 0; q < OVERLAY_REC_WORDS / 4u; q++) dst[q] = src[q];
        }
        n_list += take;
        done += take;
        if (n_list == OVERLAY_KEPT) {  // full: drain it and go on; the order is kept
          __syncthreads();
          drain(n_list);
          __syncthreads();
          n_list = 0;
        }
      }
    }
  }
  if (!had) return;
  if (n_list != 0u) {
    __syncthreads();
    drain(n_list);
  }
  if (t == 0u) atomicAdd(&A.stats[2], 1u);
  if (touched) {  // (touched implies py < dh and px < dw: a record's box lies inside the image)
    if (wide) {
      *reinterpret_cast<uint4*>(mine) = make_uint4(d0, d1, d2, d3);
    } else {
      mine[0] = d0;
      if (px + 1u < A.dw) mine[1] = d1;
      if (px + 2u < A.dw) mine[2] = d2;
      if (px + 3u < A.dw) mine[3] = d3;
    }
  }
}

}  // namespace

void launch_overlay(const OverlayLaunch& A, hipStream_t s) {
  const uint32_t tiles = A.tiles_w * A.tiles_h;
  hipLaunchKernelGGL(overlay_setup_kernel, dim3((A.n_tris + 255u) / 256u), dim3(256), 0, s, A);
  hipLaunchKernelGGL(overlay_tile_kernel, dim3(tiles), dim3(256), 0, s, A);
}

}  // namespace svr
