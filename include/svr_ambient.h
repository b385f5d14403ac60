/* svr_ambient.h — screen-space ambient occlusion over the G-buffer, applied by the lighting pass.
 *
 * svr_light_pass adds albedo * ambient to every lit pixel at full strength.  This pass estimates, per pixel, how much of
 * the hemisphere over its surface nearby geometry closes, from the depth target and the SVR_ATTR_NORMAL plane alone, and
 * writes the factor (1: open, 0: closed) to one fp32 plane; with svr_set_light_ambient_occlusion a later svr_light_pass
 * scales its ambient term by it.  It goes between the G-buffer pass and the lighting pass:
 *   svr_draw_geometry (planes) -> svr_ambient_pass -> svr_light_pass -> transparents under SVR_DEPTH_LOAD -> ...
 *
 * Output: the ambient target
 *   - One fp32 plane of the context's extent (width * height floats): the context's, allocated and zeroed by the first
 *     pass, or a caller's plane (svr_bind_ambient_target), 16-byte aligned.
 *   - The pass writes every pixel of the scissor and nothing else: colour, depth, IDs and the attribute planes are
 *     untouched, and no texel outside the scissor is read or written.  A tap outside the scissor contributes nothing.
 *
 * Inputs, taken as bound when the call is enqueued
 *   - The depth target and the current SVR_ATTR_NORMAL plane; without a normal plane: SVR_ERR_INVALID_ARGUMENT.  The
 *     albedo plane is not needed.
 *   - Depth texels must not be NaN (else the pixels are unspecified; never a fault: every LDS and global index comes from
 *     integers that were tested or clamped).
 *
 * Arithmetic, fp32
 *   - P: the pixel's world position (C17).  A pixel has a surface iff its depth is > 0, the w of its normal texel has
 *     non-zero bits and the normal's squared length is > 0; a pixel without one gets 1.
 *   - rpx = radius * pixels_per_unit / w_clip, at most SVR_AMBIENT_MAX_REACH; below one pixel the factor is 1.
 *   - SVR_AMBIENT_TAPS taps on a rotated spiral inside rpx; each tap's world position Q, v = Q - P, contributes
 *     max(v . n - bias, 0) / (v . v + 0.0001) where v . v < radius^2.
 *   - a = max(1 - intensity * radius / 8 * sum, 0), then a 5 x 5 blur that accepts the taps whose 1 / w_clip lies within
 *     sharpness (relative) of the pixel's; SVR_AMBIENT_NO_BLUR stores a itself.
 *
 * Refusals, with nothing changed: SVR_ERR_INVALID_ARGUMENT for null arguments, a parameter outside the range its field
 * names, a non-finite matrix entry, unknown flag bits, a missing normal plane; SVR_ERR_UNSUPPORTED under
 * svr_set_row_interleave with a stride above 1.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_post_pass: two kernels, out of place and idempotent.
 *     While an earlier pass's queue overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, in
 *     call order behind the replayed passes, from the addresses it was logged with; a pass that ran before the
 *     overflowing one is not run again (DESIGN.md §5 "Ambient occlusion").
 *   - The pass writes no colour: it does not flush a deferred svr_clear_color.
 *   - Caller-bound planes must stay valid and unchanged, except by operations of this context, until the next fence.
 *
 * Use by the lighting pass
 *   - include/svr_lighting.h and SvrLightPass are unchanged.  After svr_set_light_ambient_occlusion(ctx, 1) a
 *     svr_light_pass takes the ambient target current at its enqueue (none: SVR_ERR_INVALID_ARGUMENT) and C18 becomes
 *     acc = fma(c * light, sunlight_color.w, (c * ambient) * ao), ao the plane's texel at the pixel.  Off (the default):
 *     nothing changes.
 *
 * Cost: see DESIGN.md §5 "Ambient occlusion".
 *
 * Out of scope
 *   - Multiview layers, interleaved row ownership.
 *   - The sharded frame (svr_dist.h): a band rank would cut taps at its band's edge.
 *   - Bent normals, multi-bounce approximations, temporal accumulation of the factor, half-resolution evaluation.
 *
 * HIP library only: the CPU oracle has no ambient pass.
 */
#ifndef SVR_AMBIENT_H
#define SVR_AMBIENT_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SVR_AMBIENT_NO_BLUR = 1u };
#define SVR_AMBIENT_MAX_REACH 16 /* pixels: no tap is further from its pixel, in x or in y */
#define SVR_AMBIENT_TAPS 8

typedef struct SvrAmbientPass {
  float inv_viewproj[16]; /* column-major, as SvrLightPass */
  float radius;           /* world units; finite, > 0 */
  float pixels_per_unit;  /* pixels one world unit spans at clip w = 1: 0.5 * height * |proj[1][1]|; finite, > 0 */
  float bias;             /* world units; finite, >= 0 */
  float intensity;        /* finite, >= 0 */
  float sharpness;        /* blur: accepted relative difference of 1/w; finite, 0 <= s < 1 */
  uint32_t flags;         /* SVR_AMBIENT_* */
} SvrAmbientPass;         /* 88 bytes */

/* Write the ambient factor of the scissor's pixels to the ambient target (see above). */
int svr_ambient_pass(SvrContext* ctx, const SvrAmbientPass* pass);

/* A caller plane (width * height floats, 16-byte aligned) as the ambient target; NULL: back to the context's.  No fence:
 * passes already enqueued keep the plane they were enqueued with. */
int svr_bind_ambient_target(SvrContext* ctx, float* dev);

/* The current ambient target; NULL before the first pass and with nothing bound. */
int svr_get_ambient_target(SvrContext* ctx, float** dev);

/* Fences, then copies the current ambient target (bytes == width * height * 4). */
int svr_read_ambient(SvrContext* ctx, void* dst_host, size_t bytes);

/* on != 0: later svr_light_pass calls scale their ambient term by the ambient target (see above). */
int svr_set_light_ambient_occlusion(SvrContext* ctx, int on);

/* Test hook: fences, then copies the (a, 1/w_clip) scratch plane of C36 (bytes == width * height * 8; zeros outside every
 * scissor a pass has had).  SVR_ERR_INVALID_ARGUMENT before the first pass. */
int svr_debug_read_ambient_raw(SvrContext* ctx, void* dst_host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SVR_AMBIENT_H */
