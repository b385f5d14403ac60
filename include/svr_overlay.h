/* svr_overlay.h — the UI overlay pass: clipped, textured 2D triangle lists blended over the swapchain image.
 *
 * The reference's draw() ends with the blit to the swapchain image, draw_imgui onto that image, and the present.
 * svr_copy_to_swapchain is the first; svr_draw_overlay is the second: a painter for the triangle lists a UI library
 * emits.  The data layout is the one Dear ImGui's renderer backends consume (20-byte vertices, 16-bit indices, commands
 * with a clip rectangle, a texture and offsets), so an ImDrawData walks into an SvrOverlayList without conversion
 * (INTEGRATION.md "UI overlay").
 *
 * The destination is the image svr_copy_to_swapchain writes: dst_width x dst_height UNORM8 texels, rows tightly packed,
 * in either SVR_SWAPCHAIN_* format, in the caller's device memory.  Any image of that layout will do.
 *   - The context's scissor and row interleave do not apply: the commands carry their own clip rectangles.
 *   - The colour target is not touched, so a deferred svr_clear_color stays deferred.
 *   - Every texel no covered fragment reaches keeps its bits.
 *
 * Arithmetic
 *   - position: x = (pos.x - display_pos.x) * scale.x in fp32, snapped to 1/256 px: X = clamp(rintf(x * 256), -2^23, 2^23);
 *     a triangle with a non-finite x or y is dropped;
 *   - coverage: exact int64 edge functions at the pixel centres with C4's top-left rule; zero area is dropped, a negative
 *     area has vertices 1 and 2 swapped (no culling);
 *   - clip: cmin = max((clip_rect.xy - display_pos) * scale, 0), cmax = min((clip_rect.zw - display_pos) * scale, extent);
 *     the command is skipped if cmax <= cmin either way; x0 = (int32)cmin.x, x1 = x0 + (uint32)(cmax.x - cmin.x), both
 *     truncating; pixel i passes iff x0 <= i < x1, and the same in y (what the Vulkan backend's scissor does);
 *   - attributes: w1 = (float)E1 * inv, w2 = (float)E2 * inv, inv = 1.0f / (float)area; uv and the four channels of col are
 *     fmaf(w2, a2 - a0, fmaf(w1, a1 - a0, a0)); no perspective;
 *   - texel: bilinear, clamp-to-edge, no mips; texels are R | G<<8 | B<<16 | A<<24 (RGBA8) or one byte (A8: (1, 1, 1, a));
 *   - fragment: src = colour * texel; out.rgb = fmaf(src.c, src.a, dst.c * (1 - src.a)), out.a = fmaf(dst.a, 1 - src.a, src.a);
 *     the result is quantised to UNORM8 after every fragment, and the next fragment of the pixel reads what was stored;
 *   - order: fragments reach a pixel in command order, then index order: the sequential painter's result.
 *   Texture coordinates are the caller's to keep finite; whatever they are, no texel outside the texture is read.
 *
 * Refusals, with nothing changed (SVR_ERR_INVALID_ARGUMENT, the message names the offender): null arguments; a zero
 * extent or one above 16384; an unknown format; counts above the limits below; an elem_count not divisible by 3;
 * idx_offset + elem_count > n_indices; an index with vtx_offset + index >= n_vertices; a texture >= n_textures; a texture
 * with a null pointer, an unknown format or an extent outside 1..SVR_OVERLAY_MAX_TEXTURE_EXTENT; a non-finite display_pos
 * or scale, or a scale that is not > 0.  Every index is checked at the call, as svr_upload_mesh checks a mesh's: no kernel
 * can read outside the arrays.  An empty list (n_cmds == 0, or every elem_count == 0) is accepted and enqueues nothing.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged as its own kind.  The logged operation owns copies of the
 *     vertices, indices, commands and texture table: the host arrays are borrowed for the call only.
 *   - Both kernels write nothing while an earlier pass's queue overflow is pending (SVR_OPT_QUEUE_CAPS); the overlay then
 *     runs again, once, in call order behind the replayed blit.  An overlay that ran before the overflowing pass is not
 *     run again.  The image is that of blending every overlay exactly once, although the pass works in place.
 *   - The destination and the textures must stay valid until the next fence.
 *
 * Out of scope: 32-bit indices, user callbacks, sRGB blending, the RGBA16F colour target, multiview layers.
 *
 * HIP library only: the CPU oracle has no overlay pass.
 */
#ifndef SVR_OVERLAY_H
#define SVR_OVERLAY_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_OVERLAY_MAX_TRIANGLES 65536
#define SVR_OVERLAY_MAX_CMDS 4096
#define SVR_OVERLAY_MAX_TEXTURES 16
#define SVR_OVERLAY_MAX_TEXTURE_EXTENT 16384
#define SVR_OVERLAY_TEX_RGBA8 0
#define SVR_OVERLAY_TEX_A8 1
/* svr_overlay_font: this texel and its eight neighbours are fully opaque (255), so a uv at its centre,
 * ((X + 0.5) / width, (Y + 0.5) / height), samples exactly 1: the uv of untextured rectangles */
#define SVR_OVERLAY_FONT_WHITE_X 92
#define SVR_OVERLAY_FONT_WHITE_Y 43

typedef struct SvrOverlayVertex {
  float pos[2];
  float uv[2];
  uint32_t col; /* R | G<<8 | B<<16 | A<<24 */
} SvrOverlayVertex; /* 20 bytes */

typedef struct SvrOverlayCmd {
  float clip_rect[4]; /* x1, y1, x2, y2 in the units of pos */
  uint32_t texture;   /* index into SvrOverlayList.textures */
  uint32_t vtx_offset, idx_offset, elem_count;
} SvrOverlayCmd; /* 32 bytes */

typedef struct SvrOverlayTexture {
  const void* texels; /* device memory, rows tightly packed */
  uint32_t width, height, format, reserved;
} SvrOverlayTexture; /* 24 bytes */

typedef struct SvrOverlayList {
  const SvrOverlayVertex* vertices; /* host arrays, borrowed for the call */
  const uint16_t* indices;
  const SvrOverlayCmd* cmds;
  const SvrOverlayTexture* textures;
  uint32_t n_vertices, n_indices, n_cmds, n_textures;
  float display_pos[2], scale[2];
} SvrOverlayList;

typedef struct SvrOverlayStats {
  uint32_t triangles; /* submitted */
  uint32_t kept;      /* with a non-empty pixel box inside their command's clip box */
  uint32_t tiles;     /* 32x32 tiles some kept triangle's box reaches */
} SvrOverlayStats; /* of the last overlay that enqueued work */

/* Blend the list over dst (see above). */
int svr_draw_overlay(SvrContext* ctx, void* dst_dev, uint32_t dst_width, uint32_t dst_height, int dst_format, const SvrOverlayList* list);
/* The counts of the last overlay behind everything enqueued so far (a fence; a test hook).  All 0 before any. */
int svr_debug_read_overlay_stats(SvrContext* ctx, SvrOverlayStats* out);
/* The built-in A8 atlas, in host memory; needs no device.  Cells of cell_w x cell_h (6 x 8), 16 to a row, for the n_chars
 * (95) characters from first_char (32); glyphs are 5 x 7 in the cell's top left.  Digits, A-Z (lower case shares the
 * shapes), space and . , : - + % / ( ) _ are drawn; any other character is a filled box.  The 96th cell is filled whole:
 * SVR_OVERLAY_FONT_WHITE_X/Y lies in it.  Any output pointer may be null. */
int svr_overlay_font(const uint8_t** a8, uint32_t* width, uint32_t* height, uint32_t* cell_w, uint32_t* cell_h, uint32_t* first_char, uint32_t* n_chars);

#ifdef __cplusplus
}
#endif
#endif /* SVR_OVERLAY_H */
