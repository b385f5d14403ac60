// svr_overlay_text.h — a small list builder for the UI overlay pass (include/svr_overlay.h) on top of the built-in font:
// rectangles, text and windows, emitted as the vertices, 16-bit indices and commands svr_draw_overlay takes.
// simple-vk-renderer_amd/overlay.py is the same builder in Python: both make the same arrays, bit for bit, from the same
// calls.  Header only; needs nothing but the font's extents (svr_overlay_font).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/svr_overlay.h"

namespace svrhost {

struct OverlayListBuilder {
  uint32_t atlas_w, atlas_h, cell_w, cell_h, first_char, n_chars, texture;
  std::vector<SvrOverlayVertex> vertices;
  std::vector<uint16_t> indices;
  std::vector<SvrOverlayCmd> cmds;
  float white_u, white_v;

  // the extents svr_overlay_font gives; texture: the atlas's index in the texture table the list is drawn with
  OverlayListBuilder(uint32_t aw, uint32_t ah, uint32_t cw, uint32_t ch, uint32_t first, uint32_t n, uint32_t tex = 0)
      : atlas_w(aw), atlas_h(ah), cell_w(cw), cell_h(ch), first_char(first), n_chars(n), texture(tex),
        white_u(((float)SVR_OVERLAY_FONT_WHITE_X + 0.5f) / (float)aw), white_v(((float)SVR_OVERLAY_FONT_WHITE_Y + 0.5f) / (float)ah) {}

  static uint32_t pack(const uint8_t rgba[4]) { return (uint32_t)rgba[0] | ((uint32_t)rgba[1] << 8) | ((uint32_t)rgba[2] << 16) | ((uint32_t)rgba[3] << 24); }

  void command(float x0, float y0, float x1, float y1) {
    SvrOverlayCmd c{{x0, y0, x1, y1}, texture, (uint32_t)vertices.size(), (uint32_t)indices.size(), 0u};
    cmds.push_back(c);
  }
  void quad(float x0, float y0, float x1, float y1, float u0, float v0, float u1, float v1, uint32_t col) {
    if (cmds.empty()) command(0.0f, 0.0f, 16384.0f, 16384.0f);  // what is drawn outside any window
    uint32_t base = (uint32_t)vertices.size() - cmds.back().vtx_offset;
    if (base + 4u > 65536u) {  // 16-bit indices: go on in a new command with the same clip rectangle
      const SvrOverlayCmd last = cmds.back();
      command(last.clip_rect[0], last.clip_rect[1], last.clip_rect[2], last.clip_rect[3]);
      base = 0;
    }
    vertices.push_back({{x0, y0}, {u0, v0}, col});
    vertices.push_back({{x1, y0}, {u1, v0}, col});
    vertices.push_back({{x1, y1}, {u1, v1}, col});
    vertices.push_back({{x0, y1}, {u0, v1}, col});
    for (uint32_t k : {0u, 1u, 2u, 0u, 2u, 3u}) indices.push_back((uint16_t)(base + k));
    cmds.back().elem_count += 6u;
  }
  void rect(float x, float y, float w, float h, const uint8_t rgba[4]) { quad(x, y, x + w, y + h, white_u, white_v, white_u, white_v, pack(rgba)); }
  void text(float x, float y, const std::string& s, const uint8_t rgba[4], float scale = 1.0f) {
    const uint32_t col = pack(rgba);
    const float gw = (float)cell_w * scale, gh = (float)cell_h * scale;
    float px = x, py = y;
    for (unsigned char ch : s) {
      if (ch == '\n') {
        px = x;
        py = py + gh;
        continue;
      }
      uint32_t cell = (uint32_t)ch - first_char;  // (wraps below first_char: the filled cell)
      if (cell >= n_chars) cell = n_chars;
      if (ch != ' ') {
        const uint32_t cx = cell % 16u, cy = cell / 16u;
        const float u0 = (float)(cx * cell_w) / (float)atlas_w, u1 = (float)((cx + 1u) * cell_w) / (float)atlas_w;
        const float v0 = (float)(cy * cell_h) / (float)atlas_h, v1 = (float)((cy + 1u) * cell_h) / (float)atlas_h;
        quad(px, py, px + gw, py + gh, u0, v0, u1, v1, col);
      }
      px = px + gw;
    }
  }
  // a new command clipped to the window: its body, a title bar and the title; what follows is drawn inside it
  void window(float x, float y, float w, float h, const std::string& title) {
    static const uint8_t body[4] = {20, 20, 24, 200}, bar[4] = {48, 72, 120, 255}, ink[4] = {255, 255, 255, 255};
    command(x, y, x + w, y + h);
    rect(x, y, w, h, body);
    rect(x, y, w, 12.0f, bar);
    text(x + 3.0f, y + 2.0f, title, ink);
  }
  SvrOverlayList list(const SvrOverlayTexture* textures, uint32_t n_textures) const {
    SvrOverlayList l{};
    l.vertices = vertices.data();
    l.indices = indices.data();
    l.cmds = cmds.data();
    l.textures = textures;
    l.n_vertices = (uint32_t)vertices.size();
    l.n_indices = (uint32_t)indices.size();
    l.n_cmds = (uint32_t)cmds.size();
    l.n_textures = n_textures;
    l.scale[0] = l.scale[1] = 1.0f;
    return l;
  }
};

}  // namespace svrhost
