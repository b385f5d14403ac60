/* svr_attributes.h — attribute targets: what the fragment stage computed for the winning opaque fragment of each pixel.
 *
 * What a Vulkan renderer gets from further colour attachments written by the opaque pipeline: a G-buffer.  The tile kernel
 * folds barycentrics, 1/w, UV, normal, light term and unlit surface colour into one colour per pixel; with an attribute
 * plane bound it also stores them, out of the same registers.  For deferred or re-lit shading in the caller's framework,
 * normal / albedo / UV maps, texture-space work, and attribute reconstruction from {primitive, barycentrics} (svr_ids.h is
 * the other half of that visibility buffer).
 *
 * The planes.  Each is optional, row-major width * height texels of fp32 with no padding, 16-byte aligned.  The slot
 * numbers are those of svr_debug_read_trace for the same pixel.
 *   SVR_ATTR_BARY    4 floats  b1, b2 (slots 1, 2), r = 1/w (slot 3), 0.0f
 *   SVR_ATTR_UV      2 floats  u, v (slots 4, 5)
 *   SVR_ATTR_NORMAL  4 floats  nx, ny, nz (slots 15-17: interpolated, not normalised), light (slot 21)
 *   SVR_ATTR_ALBEDO  4 floats  color.rgb (slots 18-20: the interpolated vertex colour, material factor included, times the
 *                              texel), 1.0f
 *
 * Meaning
 *   - A texel holds the values of the fragment-shader invocation of the winning opaque fragment of the pixel: the fragment
 *     whose depth svr_read_depth returns, with its tie rule (the maximum over (depth, key)).  They are the very values that
 *     produced the pixel's opaque colour, not a second evaluation.
 *   - A pixel no opaque fragment won holds all-zero bits in every plane.  Transparent objects never write the planes.
 *   - b1, b2 are the screen-space (noperspective) barycentrics of the triangle that was rasterised, the weights of its
 *     second and third vertex; r is the interpolated 1/w, so a vertex attribute A is
 *     (A0/w0 + b1 (A1/w1 - A0/w0) + b2 (A2/w2 - A0/w0)) * r.  For a triangle cut by the near plane the triangle is the
 *     piece the clipper made, not the parent triangle the ID target names.
 *
 * When they are written
 *   - Every svr_draw_geometry / svr_draw_list pass clears and writes the planes over the pixels it owns (the scissor; with
 *     svr_set_row_interleave, its tile rows), exactly where it writes depth.  Other pixels are not touched.  Both colour
 *     formats, every SVR_OPT_* setting, with or without an ID target, with or without an occlusion pyramid bound (the
 *     guarantee of svr_occlusion.h carries over: the winners are the same).
 *   - svr_draw_colored_triangle, svr_draw_tex_image, svr_clear_color, svr_draw_background, depth-only passes (svr_depth.h)
 *     and multiview passes (svr_views.h) leave them untouched.
 *   - Stream-ordered like the colour, depth and ID targets: a pass writes the planes bound when it was enqueued, and so
 *     does its replay after a queue overflow (SVR_OPT_QUEUE_CAPS); the overflowed attempt writes nothing.
 *   - With no plane enabled or bound, passes run the kernels they ran before this header existed: nothing changes.
 *   - With planes, colour, depth and IDs are those of the pass without them, with one exception: under svr_set_scissor
 *     with an odd x or y, a pass without planes takes the texture derivatives of fully covered 8x8 pixel blocks from the
 *     pixels' neighbours on the wrong side (a shortcut of its tile kernel that holds for even origins only), and its
 *     colour can differ from the CPU oracle's in the last bits there.  A pass with planes does not take the shortcut on
 *     such tiles: its colour and its planes are the oracle's, and so its colour can differ from the plain pass's.
 *   - A rank of the sharded frame (svr_dist.h) writes its own rows only; planes are not exchanged.
 *
 * HIP library only: the CPU oracle has no attribute targets.
 */
#ifndef SVR_ATTRIBUTES_H
#define SVR_ATTRIBUTES_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SVR_ATTR_BARY = 1,
  SVR_ATTR_UV = 2,
  SVR_ATTR_NORMAL = 4,
  SVR_ATTR_ALBEDO = 8,
  SVR_ATTR_ALL = 15
};

/* The context-owned planes are those of `mask` from here on: bits newly set allocate their plane (zeroed) and make it the
 * target unless a caller's plane is bound; bits cleared free theirs (after a fence), and if it was the target there is
 * none from then on.  An unknown bit: SVR_ERR_INVALID_ARGUMENT.  A call that fails changes nothing. */
int svr_enable_attributes(SvrContext* ctx, uint32_t mask);
/* Caller-owned device memory (width * height texels, 16-byte aligned) as the target of ONE attribute instead of the
 * context's plane.  NULL goes back to the context's plane, or to none. */
int svr_bind_attribute_target(SvrContext* ctx, int attr, void* dev);
/* The current target of one attribute; NULL when there is none. */
int svr_get_attribute_target(SvrContext* ctx, int attr, void** dev);
/* Fences, then copies the whole plane of one attribute: `bytes` must be its size (width * height * 16, UV: * 8).
 * No such plane: SVR_ERR_INVALID_ARGUMENT. */
int svr_read_attribute(SvrContext* ctx, int attr, void* dst_host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SVR_ATTRIBUTES_H */
