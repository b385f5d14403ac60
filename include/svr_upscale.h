/* svr_upscale.h — the upscaled present: the colour target magnified to the swapchain extent with a Catmull-Rom filter, an
 * anti-ringing clamp and a contrast-adaptive sharpen.
 *
 * The reference carries a _render_scale (src/vk_engine.h:121) and sizes _draw_extent by it (src/vk_engine.cpp:1220-1222);
 * vkutil::copy_image then stretches the smaller image over the swapchain.  svr_copy_to_swapchain is that stretch, a LINEAR
 * blit.  svr_upscale_to_swapchain is a second present call for a frame rendered below the window's
 * resolution: one fused kernel (csrc/k_upscale.hip) reconstructs with a bicubic filter and sharpens at output resolution.
 * svr_copy_to_swapchain is unchanged and stays the call for identity, minifying and per-band presents.
 *
 * Source and destination
 *   - The source is the whole colour target, RGBA16F or RGBA8.  The context's scissor does not apply.
 *   - The destination is dst_width x dst_height UNORM8 texels, rows tightly packed, in either SVR_SWAPCHAIN_* format, in
 *     the caller's device memory (4-byte aligned).  The whole image is written, and no byte outside it.
 *   - W <= dst_width <= 16384 and H <= dst_height <= 16384, each axis on its own; identity on an axis is allowed.
 *
 * Arithmetic, all fp32, every operation pinned
 *   - source texel: s(x, y) is the decoded texel, each channel through sat(v) = v > 0 ? (v < 1 ? v : 1) : 0 (NaN and
 *     negatives are 0), at x clamped to [0, W-1] and y to [0, H-1];
 *   - position: C16's: su = (float)W / (float)dst_width, u = ((float)i + 0.5f) * su - 0.5f, x0 = floorf(u), t = u - x0, taps
 *     x0-1 .. x0+2; the same in y;
 *   - filter: Catmull-Rom weights in a fixed Horner form, rows first, then the four row results with the vertical weights;
 *     the result is clamped into the range of the four central texels s(x0..x0+1, y0..y0+1) (anti-ringing), all four
 *     channels alike: P;
 *   - sharpen (RGB only): over the unquantised P of the output pixel m and its neighbours n, s, e, w (indices clamped to
 *     the output image), per channel: lo / hi their minimum / maximum, a = hi > 0 ? min(lo, 1 - hi) / hi : 0, k = a * peak,
 *     O = fmaf(k, (n + s) + (e + w), m) / fmaf(4.0f, k, 1.0f), peak = -1.0f / (8.0f - 3.0f * sharpness);
 *   - store: un8(O) for RGB and un8(P) for alpha; with SVR_UPSCALE_NO_SHARPEN un8(P) for all four.
 *   With identity extents and SVR_UPSCALE_NO_SHARPEN the image is un8(sat(source)): svr_copy_to_swapchain's on a finite one.
 *
 * Refusals, with nothing changed
 *   - SVR_ERR_INVALID_ARGUMENT: null arguments; a sharpness that is not finite or outside [0, 1]; unknown flag bits; an
 *     unknown format; a zero extent or one above 16384; (svr_read_upscaled) a buffer too small;
 *   - SVR_ERR_UNSUPPORTED: a destination narrower or lower than the colour target (minification stays with
 *     svr_copy_to_swapchain); svr_set_row_interleave with a stride above 1.
 *
 * Ordering
 *   - A deferred svr_clear_color runs first, as for the blit.
 *   - Stream-ordered on the context's stream and logged as its own kind.  The kernel reads the context's overflow flag first
 *     and stores nothing while it is up; the pass is out of place and idempotent, so a replay runs it again behind the
 *     replayed passes.
 *   - It reports to the word set by svr_set_present_status as svr_copy_to_swapchain does: 0, 1 when void, 2 from a replay.
 *   - The destination must stay valid until the next fence.
 *
 * Out of scope: multiview layers; the sharded frame (include/svr_dist.h presents bands with svr_copy_to_swapchain); a
 * texture LOD bias for the lower render resolution; an sRGB transfer; temporal upscaling (history at output resolution).
 *
 * HIP library only: the CPU oracle has no upscaled present.
 */
#ifndef SVR_UPSCALE_H
#define SVR_UPSCALE_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SVR_UPSCALE_NO_SHARPEN = 1u }; /* SvrUpscalePass.flags: store the filtered, clamped image unsharpened */

typedef struct SvrUpscalePass {
  float sharpness; /* 0 .. 1: the sharpen's peak is -1 / (8 - 3 * sharpness) */
  uint32_t flags;  /* SVR_UPSCALE_* */
} SvrUpscalePass; /* 8 bytes */

/* Magnify the colour target into dst_dev (see above). */
int svr_upscale_to_swapchain(SvrContext* ctx, const SvrUpscalePass* pass, void* dst_dev, uint32_t dst_width, uint32_t dst_height,
                             int dst_format);
/* The same image into host memory, behind everything enqueued so far (a fence), as svr_read_swapchain: bytes must be at
 * least dst_width * dst_height * 4. */
int svr_read_upscaled(SvrContext* ctx, const SvrUpscalePass* pass, uint32_t dst_width, uint32_t dst_height, int dst_format,
                      void* dst_host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SVR_UPSCALE_H */
