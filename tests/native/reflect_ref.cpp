// reflect_ref — scalar restatement of the reflection pass's contract (include/svr_reflect.h) for the
// tests: one pixel at a time, no cells, no tiles, no LDS.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one; `/` and std::sqrt are correctly
// rounded (rcp_ieee is 1.0f / x).  The fp32 -> fp16 rounding is written out (h16) in ref_contract.h, with C17 and C0.
//
//   reflect_ref <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, steps, refine, resolve, frame_index, variant, pad;
//       float viewproj[16], inv_viewproj[16], camera[3], inv_z_scale, inv_z_bias, max_distance, thickness, f0, intensity,
//       distance_fade, edge_width, depth_tolerance;
//       uint16 color[H][W][4] (fp16 bit patterns); float depth[H][W]; float normal[H][W][4]; float albedo[H][W][4].
// <out>: uint16 color[H][W][4] after the pass; float trace[sh][sw][4] (C77's texels); float t_hit[sh][sw] (0 for a miss);
//       int32 hit[sh][sw][2] (the hit pixel in the target, -1 -1 for a miss).
// variant 0 is the contract.  1 .. 12 are deliberately wrong (the tests check that each one is told apart):
//   1 the normal is not normalised      2 no dither: o = 1/2 everywhere        3 the first sample is i = 0
//   4 no thickness test                 5 a sample behind but too deep ends the march
//   6 the refinement returns lo         7 rint in place of floor               8 the Fresnel exponent is 4
//   9 the edge fade is the source pixel's   10 the resolve has no depth test   11 the composite adds
//   12 a sample outside the scissor is clamped into it
#include <vector>

#include "ref_contract.h"

namespace {

struct Pass {
  uint32_t W, H, sx, sy, sw, sh, steps, refine, resolve, frame, variant, pad;
  float viewproj[16], inv_viewproj[16], cam[3], inv_z_scale, inv_z_bias, max_distance, thickness, f0, intensity, distance_fade, edge_width,
      depth_tolerance;
};
static_assert(sizeof(Pass) == 12 * 4 + 44 * 4, "the input's head");

Pass P;
int g_variant = 0;
std::vector<uint16_t> color;
std::vector<float> depth, normal, albedo;
float half_w, half_h, q_max;

// C56
uint32_t dither_hash(uint32_t x, uint32_t y, uint32_t frame) {
  uint32_t h = (x * 0x9E3779B1u) ^ (y * 0x85EBCA77u) ^ (frame * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

enum { OUTSIDE = 0, FRONT = 1, PASSED = 2, HIT = 3 };

// C75: the sample at t of the ray h0 + t dh
int sample_at(const float* h0, const float* dh, float t, int& fx, int& fy) {
  const float hx = std::fma(dh[0], t, h0[0]), hy = std::fma(dh[1], t, h0[1]), hw = std::fma(dh[3], t, h0[3]);
  if (!(hw > 0.0f)) return OUTSIDE;
  const float rw = 1.0f / hw;
  const float ux = std::fma(hx * rw, half_w, half_w), uy = std::fma(hy * rw, half_h, half_h);
  float px = g_variant == 7 ? std::rint(ux) : std::floor(ux), py = g_variant == 7 ? std::rint(uy) : std::floor(uy);
  const float x_lo = (float)P.sx, x_hi = (float)(P.sx + P.sw), y_lo = (float)P.sy, y_hi = (float)(P.sy + P.sh);
  if (!(px >= x_lo && px < x_hi && py >= y_lo && py < y_hi)) {
    if (g_variant != 12 || px != px || py != py) return OUTSIDE;
    px = px < x_lo ? x_lo : (px < x_hi ? px : x_hi - 1.0f);
    py = py < y_lo ? y_lo : (py < y_hi ? py : y_hi - 1.0f);
  }
  fx = (int)px;
  fy = (int)py;
  const float q = hw * std::fma(depth[(size_t)fy * P.W + fx], P.inv_z_scale, P.inv_z_bias);
  if (!(q >= 1.0f)) return FRONT;
  return (g_variant == 4 || q <= q_max) ? HIT : PASSED;
}

struct Traced {
  float texel[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float t_hit = 0.0f;
  int hx = -1, hy = -1;
};

// C73-C77 for the pixel (px, py) of the target
Traced trace_pixel(uint32_t px, uint32_t py) {
  Traced out;
  const size_t at = (size_t)py * P.W + px;
  // C73
  const float z = depth[at];
  const float* n = &normal[at * 4];
  const float nn = std::fma(n[2], n[2], std::fma(n[1], n[1], n[0] * n[0]));
  if (bits(albedo[at * 4 + 3]) != 0x3F800000u || bits(z) == 0u || !(nn > 0.0f)) return out;
  // C74
  float p[3];
  position(P.inv_viewproj, (float)px + 0.5f, (float)py + 0.5f, 2.0f / (float)P.W, 2.0f / (float)P.H, z, p);
  const float u[3] = {p[0] - P.cam[0], p[1] - P.cam[1], p[2] - P.cam[2]};
  const float vv = std::fma(u[2], u[2], std::fma(u[1], u[1], u[0] * u[0]));
  if (!(vv > 0.0f && vv < INFINITY)) return out;
  const float rn = g_variant == 1 ? 1.0f : 1.0f / std::sqrt(nn), rv = 1.0f / std::sqrt(vv);
  const float nh[3] = {n[0] * rn, n[1] * rn, n[2] * rn}, vh[3] = {u[0] * rv, u[1] * rv, u[2] * rv};
  const float d = std::fma(nh[2], vh[2], std::fma(nh[1], vh[1], nh[0] * vh[0]));
  const float m2d = -2.0f * d;
  const float r[3] = {std::fma(m2d, nh[0], vh[0]), std::fma(m2d, nh[1], vh[1]), std::fma(m2d, nh[2], vh[2])};
  float h0[4], dh[4];
  mat_vec(P.viewproj, p[0], p[1], p[2], 1.0f, h0);
  mat_vec(P.viewproj, r[0], r[1], r[2], 0.0f, dh);
  // C75
  const float delta = P.max_distance / (float)P.steps;
  float o = (float)(dither_hash(px, py, P.frame) >> 24) * 0x1p-8f;
  if (g_variant == 2) o = 0.5f;
  int fx = -1, fy = -1;
  float t_hit = 0.0f;
  bool found = false;
  for (uint32_t i = g_variant == 3 ? 0u : 1u; i <= P.steps; i++) {
    const float t = ((float)i + o) * delta;
    const int s = sample_at(h0, dh, t, fx, fy);
    if (s == OUTSIDE) break;
    if (s == PASSED && g_variant == 5) break;
    if (s == HIT) {
      found = true;
      t_hit = t;
      break;
    }
  }
  if (!found) return out;
  // C76
  float lo = t_hit - delta, hi = t_hit;
  for (uint32_t j = 0; j < P.refine; j++) {
    const float mid = 0.5f * (lo + hi);
    int mx, my;
    if (sample_at(h0, dh, mid, mx, my) >= PASSED) {
      hi = mid;
      fx = mx;
      fy = my;
    } else {
      lo = mid;
    }
  }
  t_hit = g_variant == 6 ? lo : hi;
  // C77
  const float m = 1.0f - sat(-d), m2 = m * m;
  const float F = std::fma(1.0f - P.f0, g_variant == 8 ? m2 * m2 : (m2 * m2) * m, P.f0);
  const float fd = sat(std::fma(-(t_hit * (1.0f / P.max_distance)), P.distance_fade, 1.0f));
  float fe = 1.0f;
  if (P.edge_width > 0.0f) {
    const int ex = g_variant == 9 ? (int)px : fx, ey = g_variant == 9 ? (int)py : fy;
    const int x0 = (int)P.sx, y0 = (int)P.sy, x1 = x0 + (int)P.sw - 1, y1 = y0 + (int)P.sh - 1;
    int e = ex - x0;
    if (x1 - ex < e) e = x1 - ex;
    if (ey - y0 < e) e = ey - y0;
    if (y1 - ey < e) e = y1 - ey;
    fe = sat(((float)e + 0.5f) * (1.0f / P.edge_width));
  }
  const float k = sat(((P.intensity * F) * fd) * fe);
  const uint16_t* c = &color[((size_t)fy * P.W + fx) * 4];
  for (int j = 0; j < 3; j++) out.texel[j] = k * san(h2f(c[j]));
  out.texel[3] = k;
  out.t_hit = t_hit;
  out.hx = fx;
  out.hy = fy;
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: reflect_ref <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  if (std::fread(&P, sizeof(P), 1, f) != 1) return 3;
  g_variant = (int)P.variant;
  if (P.sw == 0 || P.sh == 0 || P.sx + P.sw > P.W || P.sy + P.sh > P.H || P.steps < 1 || P.steps > 64 || P.refine > 8 || P.resolve > 1) return 3;
  const size_t n = (size_t)P.W * P.H;
  color.resize(n * 4);
  depth.resize(n);
  normal.resize(n * 4);
  albedo.resize(n * 4);
  if (!read_all(f, color.data(), n * 8) || !read_all(f, depth.data(), n * 4) || !read_all(f, normal.data(), n * 16) || !read_all(f, albedo.data(), n * 16))
    return 3;
  std::fclose(f);
  half_w = (float)P.W * 0.5f;
  half_h = (float)P.H * 0.5f;
  q_max = 1.0f + P.thickness;

  // ---- C73-C77: every hit reads the colour target as it was before the pass
  const size_t sn = (size_t)P.sw * P.sh;
  std::vector<float> trace(sn * 4), t_hit(sn);
  std::vector<int32_t> hit(sn * 2);
  for (uint32_t y = 0; y < P.sh; y++)
    for (uint32_t x = 0; x < P.sw; x++) {
      const Traced t = trace_pixel(P.sx + x, P.sy + y);
      const size_t at = (size_t)y * P.sw + x;
      for (int j = 0; j < 4; j++) trace[at * 4 + j] = t.texel[j];
      t_hit[at] = t.t_hit;
      hit[at * 2] = t.hx;
      hit[at * 2 + 1] = t.hy;
    }

  // ---- C78, C79.  (intensity == 0: decided at the call, the target keeps its bits)
  auto iz = [&](uint32_t x, uint32_t y) { return std::fma(depth[(size_t)(P.sy + y) * P.W + P.sx + x], P.inv_z_scale, P.inv_z_bias); };
  for (uint32_t y = 0; y < (P.intensity == 0.0f ? 0u : P.sh); y++)
    for (uint32_t x = 0; x < P.sw; x++) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ws = 0.0f;
      if (P.resolve == 0) {
        for (int j = 0; j < 4; j++) acc[j] = trace[((size_t)y * P.sw + x) * 4 + j];
        ws = 1.0f;
      } else {
        const float izc = iz(x, y), tol = P.depth_tolerance * izc;
        for (int dy = -1; dy <= 1; dy++)
          for (int dx = -1; dx <= 1; dx++) {
            const uint32_t tx = clampi((int64_t)x + dx, P.sw), ty = clampi((int64_t)y + dy, P.sh);
            if (!((dx == 0 && dy == 0) || g_variant == 10 || std::fabs(iz(tx, ty) - izc) <= tol)) continue;
            for (int j = 0; j < 4; j++) acc[j] = acc[j] + trace[((size_t)ty * P.sw + tx) * 4 + j];
            ws = ws + 1.0f;
          }
      }
      const float rws = 1.0f / ws, kb = acc[3] * rws;
      uint16_t* px = &color[((size_t)(P.sy + y) * P.W + P.sx + x) * 4];
      for (int j = 0; j < 3; j++) {
        const float I = san(h2f(px[j]));
        px[j] = h16(san(std::fma(acc[j], rws, g_variant == 11 ? I : std::fma(-kb, I, I))));
      }
    }

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(color.data(), 2, color.size(), f);
  std::fwrite(trace.data(), 4, trace.size(), f);
  std::fwrite(t_hit.data(), 4, t_hit.size(), f);
  std::fwrite(hit.data(), 4, hit.size(), f);
  return std::fclose(f) == 0 ? 0 : 4;
}
