// ambient_ref — scalar restatement of the ambient pass's contract for the tests, and of the lighting
// contract (C17-C19) with the ambient factor of include/svr_ambient.h.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.  The tap tables are the kernel's
// (csrc/svr_ambient_tables.h: literals); C17 and the lighting chain of one pixel are ref_contract.h's.
//
//   ambient_ref ao <in> <out>
// <in>  (little endian): uint32 W, H, sx, sy, sw, sh, flags; float inv_viewproj[16], radius, pixels_per_unit, bias,
//       intensity, sharpness; float depth[H][W], normal[H][W][4].
// <out>: float raw[H][W][2] (C36's (a, 1/w)), float out[H][W] (C37), both zero outside the scissor; uint8 kind[H][W]:
//        0 outside the scissor, 1 no surface, 2 rpx below one pixel, 3 evaluated, 4 evaluated at the reach cap.
//        Bits 16-23 of flags name a deliberately wrong variant of one rule (0: the contract; the list is at run_ao), for
//        tests/test_ambient_ref.py to show that the fp64 statement of tests/ambient_ref.py catches each.
//
//   ambient_ref light <in> <out>
// <in>  as tests/native/light_ref.cpp's, then float ao[H][W].  <out>: as light_ref's.  acc starts from
//       fma(c * light, sun_color.w, (c * ambient) * ao).
//
//   ambient_ref tables <out>
// <out>: float D[8][2], R[16][2], f[8]: the tables and the radius fractions of C34.
#include <vector>

#include "../../simple-vk-renderer_amd/csrc/svr_ambient_tables.h"
#include "ref_contract.h"

namespace {

float fraction(int k) { return ((float)((3 * k) & 7) + 0.5f) * 0.125f; }

// the wrong variants (bits 16-23 of flags): one rule each, everything else the contract's
enum Variant : uint32_t {
  V_NONE = 0,
  V_ROTATION_FROM_SCISSOR = 1,  // the rotation indexed by scissor-relative coordinates
  V_FRACTION_FROM_K = 2,        // f_k from k instead of 3k & 7
  V_TRUNCATE = 3,               // rintf replaced by truncation
  V_TAP_AT_CORNER = 4,          // the tap unprojected at its texel's corner
  V_TAP_CLAMPED_IN = 5,         // a tap outside the scissor clamped in instead of dropped
  V_NORMAL_AS_STORED = 6,       // the normal not normalised
  V_BIAS_ADDED = 7,
  V_NO_RANGE_TEST = 8,
  V_BLUR_CLAMPED_TO_IMAGE = 9,  // the blur's coordinates clamped to the image instead of the scissor
  V_BLUR_ABSOLUTE = 10,         // the blur accepts |hw_t - hw_c| <= sharpness
  V_BLUR_3X3 = 11,
  V_REACH_8 = 12,               // the reach cap at 8
  V_COUNT
};

int run_tables(const char* out_path) {
  FILE* o = std::fopen(out_path, "wb");
  if (!o) return 4;
  float f[8];
  for (int k = 0; k < 8; k++) f[k] = fraction(k);
  bool ok = std::fwrite(SVR_AMBIENT_D, 4, 16, o) == 16 && std::fwrite(SVR_AMBIENT_R, 4, 32, o) == 32 && std::fwrite(f, 4, 8, o) == 8;
  ok = std::fclose(o) == 0 && ok;
  return ok ? 0 : 4;
}

int run_ao(const char* in_path, const char* out_path) {
  FILE* f = std::fopen(in_path, "rb");
  if (!f) return 2;
  uint32_t hdr[7];
  float inv_vp[16], par[5];
  if (!read_all(f, hdr, sizeof hdr) || !read_all(f, inv_vp, sizeof inv_vp) || !read_all(f, par, sizeof par)) return 3;
  const uint32_t W = hdr[0], H = hdr[1], sx = hdr[2], sy = hdr[3], sw = hdr[4], sh = hdr[5], flags = hdr[6] & 0xffffu;
  const uint32_t variant = (hdr[6] >> 16) & 0xffu;
  if (variant >= V_COUNT || (hdr[6] >> 24)) return 3;
  const float radius = par[0], ppu = par[1], bias = par[2], intensity = par[3], sharpness = par[4];
  const size_t n = (size_t)W * H;
  std::vector<float> depth(n), normal(n * 4);
  if (!read_all(f, depth.data(), n * 4) || !read_all(f, normal.data(), n * 16)) return 3;
  std::fclose(f);
  if (sx + sw > W || sy + sh > H) return 3;

  // taken once, on the host (C33, C35, C36)
  const float radius_px = radius * ppu, radius2 = radius * radius, coef = (intensity * radius) * 0.125f;
  const float kx = 2.0f / (float)W, ky = 2.0f / (float)H;
  std::vector<float> raw(n * 2, 0.0f), out(n, 0.0f);
  std::vector<uint8_t> kind(n, 0);
  for (uint32_t py = sy; py < sy + sh; py++) {
    for (uint32_t px = sx; px < sx + sw; px++) {
      const size_t i = (size_t)py * W + px;
      // C32
      const float z = depth[i];
      const float* nr = &normal[i * 4];
      float h[4];
      unproject(inv_vp, (float)px + 0.5f, (float)py + 0.5f, kx, ky, z, h);
      const float nn = std::fma(nr[2], nr[2], std::fma(nr[1], nr[1], nr[0] * nr[0]));
      if (!(z > 0.0f && bits(nr[3]) != 0u && nn > 0.0f)) {
        raw[i * 2] = 1.0f;
        raw[i * 2 + 1] = 0.0f;
        kind[i] = 1;
        continue;
      }
      float P[3];
      divide_w(h, P);
      const float rl = 1.0f / std::sqrt(nn);
      const float nh[3] = {nr[0] * rl, nr[1] * rl, nr[2] * rl};
      const float* nu = variant == V_NORMAL_AS_STORED ? nr : nh;
      // C33
      float rpx = radius_px * h[3];
      const float cap = variant == V_REACH_8 ? 8.0f : 16.0f;
      rpx = rpx < cap ? rpx : cap;
      if (!(rpx >= 1.0f)) {
        raw[i * 2] = 1.0f;
        raw[i * 2 + 1] = h[3];
        kind[i] = 2;
        continue;
      }
      kind[i] = rpx == cap ? 4 : 3;
      // C34
      const uint32_t rx = variant == V_ROTATION_FROM_SCISSOR ? px - sx : px, ry = variant == V_ROTATION_FROM_SCISSOR ? py - sy : py;
      const float* rot = SVR_AMBIENT_R[(ry & 3u) * 4u + (rx & 3u)];
      float sum = 0.0f;
      for (int k = 0; k < 8; k++) {
        const float dx = SVR_AMBIENT_D[k][0], dy = SVR_AMBIENT_D[k][1];
        const float ux = dx * rot[0] - dy * rot[1], uy = std::fma(dx, rot[1], dy * rot[0]);
        const float rf = rpx * (variant == V_FRACTION_FROM_K ? ((float)k + 0.5f) * 0.125f : fraction(k));
        const float ox = variant == V_TRUNCATE ? std::trunc(rf * ux) : std::rint(rf * ux);
        const float oy = variant == V_TRUNCATE ? std::trunc(rf * uy) : std::rint(rf * uy);
        if (ox == 0.0f && oy == 0.0f) continue;
        long tx = (long)px + (long)ox, ty = (long)py + (long)oy;
        if (variant == V_TAP_CLAMPED_IN) {
          tx = tx < (long)sx ? (long)sx : (tx > (long)(sx + sw) - 1 ? (long)(sx + sw) - 1 : tx);
          ty = ty < (long)sy ? (long)sy : (ty > (long)(sy + sh) - 1 ? (long)(sy + sh) - 1 : ty);
        }
        if (tx < (long)sx || tx >= (long)(sx + sw) || ty < (long)sy || ty >= (long)(sy + sh)) continue;
        const float zt = depth[(size_t)ty * W + (size_t)tx];
        if (!(zt > 0.0f)) continue;
        // C35
        float g[3];
        const float centre = variant == V_TAP_AT_CORNER ? 0.0f : 0.5f;
        position(inv_vp, (float)tx + centre, (float)ty + centre, kx, ky, zt, g);
        const float vx = g[0] - P[0], vy = g[1] - P[1], vz = g[2] - P[2];
        const float vv = std::fma(vz, vz, std::fma(vy, vy, vx * vx));
        if (!(vv < radius2) && variant != V_NO_RANGE_TEST) continue;
        const float vn = std::fma(vz, nu[2], std::fma(vy, nu[1], vx * nu[0])) - (variant == V_BIAS_ADDED ? -bias : bias);
        sum = sum + (vn > 0.0f ? vn : 0.0f) / (vv + 0.0001f);
      }
      // C36
      float a = 1.0f - coef * sum;
      a = a > 0.0f ? a : 0.0f;
      raw[i * 2] = a;
      raw[i * 2 + 1] = h[3];
    }
  }
  // C37
  for (uint32_t py = sy; py < sy + sh; py++) {
    for (uint32_t px = sx; px < sx + sw; px++) {
      const size_t i = (size_t)py * W + px;
      if (flags & 1u) {
        out[i] = raw[i * 2];
        continue;
      }
      const float hc = raw[i * 2 + 1];
      if (bits(hc) == 0u) {
        out[i] = 1.0f;
        continue;
      }
      const float lim = variant == V_BLUR_ABSOLUTE ? sharpness : sharpness * hc;
      const long bx0 = variant == V_BLUR_CLAMPED_TO_IMAGE ? 0 : (long)sx, bx1 = variant == V_BLUR_CLAMPED_TO_IMAGE ? (long)W : (long)(sx + sw);
      const long by0 = variant == V_BLUR_CLAMPED_TO_IMAGE ? 0 : (long)sy, by1 = variant == V_BLUR_CLAMPED_TO_IMAGE ? (long)H : (long)(sy + sh);
      const int br = variant == V_BLUR_3X3 ? 1 : 2;
      float sum = 0.0f;
      uint32_t count = 0;
      for (int dy = -br; dy <= br; dy++) {
        for (int dx = -br; dx <= br; dx++) {
          long tx = (long)px + dx, ty = (long)py + dy;
          tx = tx < bx0 ? bx0 : (tx > bx1 - 1 ? bx1 - 1 : tx);
          ty = ty < by0 ? by0 : (ty > by1 - 1 ? by1 - 1 : ty);
          const size_t j = (size_t)ty * W + (size_t)tx;
          if ((dx == 0 && dy == 0) || std::fabs(raw[j * 2 + 1] - hc) <= lim) {
            sum = sum + raw[j * 2];
            count++;
          }
        }
      }
      out[i] = sum / (float)count;
    }
  }
  FILE* o = std::fopen(out_path, "wb");
  if (!o) return 4;
  bool ok = std::fwrite(raw.data(), 4, raw.size(), o) == raw.size() && std::fwrite(out.data(), 4, n, o) == n && std::fwrite(kind.data(), 1, n, o) == n;
  ok = std::fclose(o) == 0 && ok;
  return ok ? 0 : 4;
}

int run_light(const char* in_path, const char* out_path) {
  FILE* f = std::fopen(in_path, "rb");
  if (!f) return 2;
  LightFrame F;
  if (!read_all(f, &F, sizeof F)) return 3;
  const uint32_t W = F.W, H = F.H;
  const size_t n = (size_t)W * H;
  std::vector<Light> lights(F.n_lights);
  std::vector<float> depth(n), normal(n * 4), albedo(n * 4), shadow((size_t)F.Ws * F.Hs), ao(n);
  if (!read_all(f, lights.data(), lights.size() * sizeof(Light)) || !read_all(f, depth.data(), n * 4) || !read_all(f, normal.data(), n * 16) ||
      !read_all(f, albedo.data(), n * 16) || !read_all(f, shadow.data(), shadow.size() * 4) || !read_all(f, ao.data(), n * 4))
    return 3;
  std::fclose(f);

  std::vector<float> rgba(n * 4, 0.0f), position(n * 3, 0.0f);
  std::vector<uint8_t> winner(n, 0), in_shadow(n, 0);
  for (uint32_t py = 0; py < H; py++) {
    for (uint32_t px = 0; px < W; px++) {
      const size_t i = (size_t)py * W + px;
      if (bits(albedo[i * 4 + 3]) != 0x3F800000u) continue;
      winner[i] = 1;
      bool shadowed;  // C17-C19, with the ambient factor
      light_pixel(F, lights.data(), shadow.data(), px, py, depth[i], &normal[i * 4], &albedo[i * 4], &ao[i], &position[i * 3], shadowed, &rgba[i * 4]);
      in_shadow[i] = shadowed ? 1 : 0;
      rgba[i * 4 + 3] = 1.0f;
    }
  }
  FILE* o = std::fopen(out_path, "wb");
  if (!o) return 4;
  bool ok = std::fwrite(rgba.data(), 4, rgba.size(), o) == rgba.size() && std::fwrite(winner.data(), 1, n, o) == n &&
            std::fwrite(position.data(), 4, position.size(), o) == position.size() && std::fwrite(in_shadow.data(), 1, n, o) == n;
  ok = std::fclose(o) == 0 && ok;
  return ok ? 0 : 4;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "tables")) return run_tables(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "ao")) return run_ao(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "light")) return run_light(argv[2], argv[3]);
  std::fprintf(stderr, "usage: ambient_ref ao|light <in> <out> | ambient_ref tables <out>\n");
  return 2;
}
