// overlay_ref.cpp — the sequential painter of DESIGN.md C43-C49 (include/svr_overlay.h) as a scalar program: for each
// command, each of its triangles and each pixel of the triangle's box, the integer coverage test and the fp32 chain,
// spelled with the fmaf()s the contract names.  Build with -ffp-contract=off.
//
//   overlay_ref in.bin out.bin
// in:  uint32 {width, height, format, variant, n_vertices, n_indices, n_cmds, n_textures}, float {display_pos[2], scale[2]},
//      the vertices (20 bytes each), the indices (uint16, padded to 4 bytes), the commands (32 bytes each), per texture
//      uint32 {width, height, format, 0} and its texels (padded to 4 bytes), then the image (uint32 per texel).
// out: the image, a uint32 per pixel counting the fragments that reached it, uint32 {triangles, kept, tiles}.
// variant: 0 is the contract; 1..9 are the wrong painters tests/test_overlay_ref.py must tell from it.
#include <algorithm>
#include <vector>

#include "ref_contract.h"  // clampi, the int overload

namespace {

enum { MIRRORED_TOP_LEFT = 1, CORNERS = 2, NO_QUANTISE = 3, REVERSED = 4, CLIP_ROUNDED = 5, SWAP_RB = 6, A8_GREY = 7, WRAP = 8, PREMULTIPLIED = 9 };

struct Vertex { float pos[2], uv[2]; uint32_t col; };
struct Cmd { float clip[4]; uint32_t texture, vtx_offset, idx_offset, elem_count; };
struct Texture { uint32_t w, h, format; std::vector<uint8_t> texels; };
static_assert(sizeof(Vertex) == 20 && sizeof(Cmd) == 32, "the layouts of include/svr_overlay.h");

const float kInv255 = 0x1.010102p-8f;
float chan(uint32_t t, int c) { return (float)((t >> (8 * c)) & 0xffu) * kInv255; }
uint32_t un8(float f) { return (uint32_t)lrintf(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f); }

int64_t snap(float x) { return (int64_t)fminf(fmaxf(rintf(x * 256.0f), -8388608.0f), 8388608.0f); }

int wrapi(int v, int n) { return ((v % n) + n) % n; }

void tap(float coord, uint32_t extent, int variant, int& i0, int& i1, float& frac) {
  const float s = coord * (float)extent - 0.5f, fs = floorf(s);
  frac = s - fs;
  const int i = (int)fminf(fmaxf(fs, -1.0f), (float)extent);
  i0 = variant == WRAP ? wrapi(i, (int)extent) : clampi(i, (int)extent);
  i1 = variant == WRAP ? wrapi(i + 1, (int)extent) : clampi(i + 1, (int)extent);
}
float filt(float a, float b, float c00, float c10, float c01, float c11) {
  const float top = fmaf(a, c10 - c00, c00), bot = fmaf(a, c11 - c01, c01);
  return fmaf(b, bot - top, top);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t hdr[8];
  float par[4];
  if (fread(hdr, 4, 8, f) != 8 || fread(par, 4, 4, f) != 4) return 2;
  const uint32_t W = hdr[0], H = hdr[1], format = hdr[2];
  const int variant = (int)hdr[3];
  const uint32_t n_vtx = hdr[4], n_idx = hdr[5], n_cmds = hdr[6], n_tex = hdr[7];
  std::vector<Vertex> vtx(n_vtx);
  std::vector<uint16_t> idx((n_idx + 1u) & ~1u);
  std::vector<Cmd> cmds(n_cmds);
  if (n_vtx && fread(vtx.data(), sizeof(Vertex), n_vtx, f) != n_vtx) return 2;
  if (!idx.empty() && fread(idx.data(), 2, idx.size(), f) != idx.size()) return 2;
  if (n_cmds && fread(cmds.data(), sizeof(Cmd), n_cmds, f) != n_cmds) return 2;
  std::vector<Texture> tex(n_tex);
  for (Texture& t : tex) {
    uint32_t th[4];
    if (fread(th, 4, 4, f) != 4) return 2;
    t.w = th[0]; t.h = th[1]; t.format = th[2];
    const size_t bytes = ((size_t)t.w * t.h * (t.format == 1 ? 1 : 4) + 3u) & ~(size_t)3u;
    t.texels.resize(bytes);
    if (fread(t.texels.data(), 1, bytes, f) != bytes) return 2;
  }
  std::vector<uint32_t> img((size_t)W * H), count((size_t)W * H, 0u);
  if (fread(img.data(), 4, img.size(), f) != img.size()) return 2;
  fclose(f);
  std::vector<float> held;  // NO_QUANTISE: the unrounded colour of the pixels touched so far
  std::vector<uint8_t> touched;
  if (variant == NO_QUANTISE) { held.resize(img.size() * 4); touched.assign(img.size(), 0); }

  const bool bgr = (format == 0) != (variant == SWAP_RB);  // SVR_SWAPCHAIN_B8G8R8A8 = 0
  const int rc = bgr ? 2 : 0, bc = bgr ? 0 : 2;
  const uint32_t tiles_x = (W + 31u) / 32u, tiles_y = (H + 31u) / 32u;
  std::vector<uint8_t> tile_hit((size_t)tiles_x * tiles_y, 0);
  uint32_t submitted = 0, kept = 0;
  const float ext[2] = {(float)W, (float)H};

  for (uint32_t cc = 0; cc < n_cmds; cc++) {
    const Cmd& cmd = cmds[variant == REVERSED ? n_cmds - 1u - cc : cc];
    const uint32_t n_tri = cmd.elem_count / 3u;
    submitted += n_tri;
    if (n_tri == 0) continue;
    // C45
    int64_t c0[2], c1[2];
    bool empty = false;
    for (int k = 0; k < 2; k++) {
      float cmin = (cmd.clip[k] - par[k]) * par[2 + k], cmax = (cmd.clip[2 + k] - par[k]) * par[2 + k];
      if (cmin < 0.0f) cmin = 0.0f;
      if (cmax > ext[k]) cmax = ext[k];
      if (!(cmax > cmin)) { empty = true; break; }
      if (variant == CLIP_ROUNDED) {
        c0[k] = (int64_t)lrintf(cmin);
        c1[k] = c0[k] + (int64_t)lrintf(cmax - cmin);
      } else {
        c0[k] = (int64_t)(int32_t)cmin;
        c1[k] = c0[k] + (int64_t)(uint32_t)(cmax - cmin);
      }
      if (c1[k] > (int64_t)(k ? H : W)) c1[k] = (int64_t)(k ? H : W);
    }
    if (empty) continue;
    const Texture& T = tex[cmd.texture];
    for (uint32_t tt = 0; tt < n_tri; tt++) {
      const uint32_t tri = variant == REVERSED ? n_tri - 1u - tt : tt;
      // C43
      int64_t X[3], Y[3];
      float u[3], v[3];
      uint32_t col[3];
      bool ok = true;
      for (int k = 0; k < 3; k++) {
        const Vertex& w = vtx[cmd.vtx_offset + idx[cmd.idx_offset + 3u * tri + k]];
        const float x = (w.pos[0] - par[0]) * par[2], y = (w.pos[1] - par[1]) * par[3];
        ok = ok && std::isfinite(x) && std::isfinite(y);
        X[k] = snap(x); Y[k] = snap(y);
        u[k] = w.uv[0]; v[k] = w.uv[1]; col[k] = w.col;
      }
      if (!ok) continue;
      // C44
      int64_t area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
      if (area == 0) continue;
      if (area < 0) {
        area = -area;
        std::swap(X[1], X[2]); std::swap(Y[1], Y[2]); std::swap(u[1], u[2]); std::swap(v[1], v[2]); std::swap(col[1], col[2]);
      }
      const int64_t minx = std::min(X[0], std::min(X[1], X[2])), maxx = std::max(X[0], std::max(X[1], X[2]));
      const int64_t miny = std::min(Y[0], std::min(Y[1], Y[2])), maxy = std::max(Y[0], std::max(Y[1], Y[2]));
      const int64_t half = variant == CORNERS ? 0 : 128;
      // floor division by 256 is an arithmetic shift
      const int64_t x0 = std::max((minx - half + 255) >> 8, c0[0]), x1 = std::min(((maxx - half) >> 8) + 1, c1[0]);
      const int64_t y0 = std::max((miny - half + 255) >> 8, c0[1]), y1 = std::min(((maxy - half) >> 8) + 1, c1[1]);
      if (x1 <= x0 || y1 <= y0) continue;
      kept++;
      for (int64_t ty = y0 / 32; ty <= (y1 - 1) / 32; ty++)
        for (int64_t tx = x0 / 32; tx <= (x1 - 1) / 32; tx++) tile_hit[(size_t)ty * tiles_x + (size_t)tx] = 1;
      const float inv = 1.0f / (float)area;
      int64_t dx[3], dy[3], bias[3];
      for (int k = 0; k < 3; k++) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        dx[k] = X[b] - X[a]; dy[k] = Y[b] - Y[a];
        const bool top_left = variant == MIRRORED_TOP_LEFT ? (dy[k] > 0 || (dy[k] == 0 && dx[k] < 0)) : (dy[k] < 0 || (dy[k] == 0 && dx[k] > 0));
        bias[k] = top_left ? 0 : -1;
      }
      for (int64_t j = y0; j < y1; j++)
        for (int64_t i = x0; i < x1; i++) {
          const int64_t Px = 256 * i + half, Py = 256 * j + half;
          int64_t e[3];
          bool in = true;
          for (int k = 0; k < 3; k++) {
            const int a = (k + 1) % 3;
            e[k] = dx[k] * (Py - Y[a]) - dy[k] * (Px - X[a]);
            in = in && e[k] + bias[k] >= 0;
          }
          if (!in) continue;
          const size_t p = (size_t)j * W + (size_t)i;
          count[p]++;
          // C46
          const float w1 = (float)e[1] * inv, w2 = (float)e[2] * inv;
          auto attr = [&](float a0, float a1, float a2) { return fmaf(w2, a2 - a0, fmaf(w1, a1 - a0, a0)); };
          const float uu = attr(u[0], u[1], u[2]), vv = attr(v[0], v[1], v[2]);
          float c[4];
          for (int k = 0; k < 4; k++) c[k] = attr(chan(col[0], k), chan(col[1], k), chan(col[2], k));
          // C47
          int i0, i1, j0, j1;
          float a, b;
          tap(uu, T.w, variant, i0, i1, a);
          tap(vv, T.h, variant, j0, j1, b);
          float t[4];
          if (T.format == 1) {
            auto at = [&](int x, int y) { return chan(T.texels[(size_t)y * T.w + x], 0); };
            const float al = filt(a, b, at(i0, j0), at(i1, j0), at(i0, j1), at(i1, j1));
            t[0] = t[1] = t[2] = variant == A8_GREY ? al : 1.0f;
            t[3] = al;
          } else {
            const uint32_t* px = reinterpret_cast<const uint32_t*>(T.texels.data());
            const uint32_t t00 = px[(size_t)j0 * T.w + i0], t10 = px[(size_t)j0 * T.w + i1], t01 = px[(size_t)j1 * T.w + i0], t11 = px[(size_t)j1 * T.w + i1];
            for (int k = 0; k < 4; k++) t[k] = filt(a, b, chan(t00, k), chan(t10, k), chan(t01, k), chan(t11, k));
          }
          // C48
          const float sr = c[0] * t[0], sg = c[1] * t[1], sb = c[2] * t[2], sa = c[3] * t[3];
          const float ia = 1.0f - sa;
          float d[4];  // r, g, b, a
          if (variant == NO_QUANTISE && touched[p]) {
            std::memcpy(d, &held[p * 4], sizeof(d));
          } else {
            d[0] = chan(img[p], rc); d[1] = chan(img[p], 1); d[2] = chan(img[p], bc); d[3] = chan(img[p], 3);
          }
          float o[4];
          if (variant == PREMULTIPLIED) {
            o[0] = fmaf(d[0], ia, sr); o[1] = fmaf(d[1], ia, sg); o[2] = fmaf(d[2], ia, sb);
          } else {
            o[0] = fmaf(sr, sa, d[0] * ia); o[1] = fmaf(sg, sa, d[1] * ia); o[2] = fmaf(sb, sa, d[2] * ia);
          }
          o[3] = fmaf(d[3], ia, sa);
          if (variant == NO_QUANTISE) {
            std::memcpy(&held[p * 4], o, sizeof(o));
            touched[p] = 1;
          }
          img[p] = (un8(o[0]) << (8 * rc)) | (un8(o[1]) << 8) | (un8(o[2]) << (8 * bc)) | (un8(o[3]) << 24);
        }
    }
  }
  uint32_t tiles = 0;
  for (uint8_t h : tile_hit) tiles += h;
  const uint32_t stats[3] = {submitted, kept, tiles};
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(img.data(), 4, img.size(), f);
  fwrite(count.data(), 4, count.size(), f);
  fwrite(stats, 4, 3, f);
  fclose(f);
  return 0;
}
