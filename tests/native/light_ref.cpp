// light_ref — scalar, brute-force restatement of the lighting contract for the tests: every light is
// visited at every pixel, no tiles, no culling.  Built by the tests with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math
// so every operation below is one IEEE fp32 operation and std::fma the only fused one.
//
//   light_ref <in> <out>
// <in>  (little endian): uint32 W, H, n_lights, Ws, Hs (Ws = Hs = 0: no shadow map); float inv_viewproj[16], ambient[4],
//       sun_direction[4], sun_color[4], shadow_viewproj[16], shadow_bias; n_lights x {float position[3], radius, color[3],
//       intensity}; float depth[H][W], normal[H][W][4], albedo[H][W][4], shadow[Hs][Ws].
// <out>: float rgba[H][W][4] (zeros where no winner); uint8 winner[H][W]; float position[H][W][3]; uint8 shadowed[H][W].
// The stores of C20 are the Python side's (numpy casts).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Light {
  float pos[3], radius, color[3], intensity;
};

bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

// column-major matrix times (x, y, z, w), the C0 chain
void mat_vec(const float* m, float x, float y, float z, float w, float out[4]) {
  for (int r = 0; r < 4; r++) {
    float a = m[r] * x;
    a = std::fma(m[4 + r], y, a);
    a = std::fma(m[8 + r], z, a);
    a = std::fma(m[12 + r], w, a);
    out[r] = a;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: light_ref <in> <out>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[5];
  float inv_vp[16], ambient[4], sun_dir[4], sun_color[4], shadow_vp[16], bias;
  if (!read_all(f, hdr, sizeof hdr) || !read_all(f, inv_vp, sizeof inv_vp) || !read_all(f, ambient, sizeof ambient) ||
      !read_all(f, sun_dir, sizeof sun_dir) || !read_all(f, sun_color, sizeof sun_color) || !read_all(f, shadow_vp, sizeof shadow_vp) ||
      !read_all(f, &bias, sizeof bias))
    return 3;
  const uint32_t W = hdr[0], H = hdr[1], n_lights = hdr[2], Ws = hdr[3], Hs = hdr[4];
  const size_t n = (size_t)W * H;
  std::vector<Light> lights(n_lights);
  std::vector<float> depth(n), normal(n * 4), albedo(n * 4), shadow((size_t)Ws * Hs);
  if (!read_all(f, lights.data(), lights.size() * sizeof(Light)) || !read_all(f, depth.data(), n * 4) || !read_all(f, normal.data(), n * 16) ||
      !read_all(f, albedo.data(), n * 16) || !read_all(f, shadow.data(), shadow.size() * 4))
    return 3;
  std::fclose(f);

  std::vector<float> rgba(n * 4, 0.0f), position(n * 3, 0.0f);
  std::vector<uint8_t> winner(n, 0), in_shadow(n, 0);
  const float kx = 2.0f / (float)W, ky = 2.0f / (float)H;
  for (uint32_t py = 0; py < H; py++) {
    for (uint32_t px = 0; px < W; px++) {
      const size_t i = (size_t)py * W + px;
      uint32_t wbits;
      std::memcpy(&wbits, &albedo[i * 4 + 3], 4);
      if (wbits != 0x3F800000u) continue;
      winner[i] = 1;
      const float* nrm = &normal[i * 4];
      const float* c = &albedo[i * 4];
      // C17
      const float xn = std::fma((float)px + 0.5f, kx, -1.0f), yn = std::fma((float)py + 0.5f, ky, -1.0f);
      float h[4];
      mat_vec(inv_vp, xn, yn, depth[i], 1.0f, h);
      const float rw = 1.0f / h[3];
      const float p[3] = {h[0] * rw, h[1] * rw, h[2] * rw};
      std::memcpy(&position[i * 3], p, 12);
      // C18
      const float d = std::fma(nrm[2], sun_dir[2], std::fma(nrm[1], sun_dir[1], nrm[0] * sun_dir[0]));
      bool shadowed = false;
      if (Ws) {
        float q[4];
        mat_vec(shadow_vp, p[0], p[1], p[2], 1.0f, q);
        const float rq = 1.0f / q[3];
        const float sx = std::fma(q[0] * rq, (float)Ws / 2.0f, (float)Ws / 2.0f);
        const float sy = std::fma(q[1] * rq, (float)Hs / 2.0f, (float)Hs / 2.0f);
        const float sz = q[2] * rq;
        const float fx = std::floor(sx), fy = std::floor(sy);
        if (q[3] > 0.0f && 0.0f <= fx && fx < (float)Ws && 0.0f <= fy && fy < (float)Hs)
          shadowed = sz + bias < shadow[(size_t)fy * Ws + (size_t)fx];
      }
      in_shadow[i] = shadowed ? 1 : 0;
      const float light = shadowed ? 0.1f : std::fmax(d, 0.1f);
      float acc[3];
      for (int ch = 0; ch < 3; ch++) acc[ch] = std::fma(c[ch] * light, sun_color[3], c[ch] * ambient[ch]);
      // C19
      for (uint32_t l = 0; l < n_lights; l++) {
        const Light& pl = lights[l];
        const float vx = pl.pos[0] - p[0], vy = pl.pos[1] - p[1], vz = pl.pos[2] - p[2];
        const float d2 = std::fma(vz, vz, std::fma(vy, vy, vx * vx));
        const float r2 = pl.radius * pl.radius;
        if (!(d2 < r2)) continue;
        const float ndl = std::fma(nrm[2], vz, std::fma(nrm[1], vy, nrm[0] * vx));
        if (!(ndl > 0.0f)) continue;
        const float t = 1.0f - d2 / r2;
        const float k = ((ndl / std::sqrt(d2)) * ((t * t) / (d2 + 1.0f))) * pl.intensity;
        for (int ch = 0; ch < 3; ch++) acc[ch] = std::fma(c[ch] * pl.color[ch], k, acc[ch]);
      }
      rgba[i * 4 + 0] = acc[0];
      rgba[i * 4 + 1] = acc[1];
      rgba[i * 4 + 2] = acc[2];
      rgba[i * 4 + 3] = 1.0f;
    }
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  bool ok = std::fwrite(rgba.data(), 4, rgba.size(), o) == rgba.size() && std::fwrite(winner.data(), 1, n, o) == n &&
            std::fwrite(position.data(), 4, position.size(), o) == position.size() && std::fwrite(in_shadow.data(), 1, n, o) == n;
  ok = std::fclose(o) == 0 && ok;
  return ok ? 0 : 4;
}
