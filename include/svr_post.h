/* svr_post.h — the HDR post pass: exposure, bloom and a tone-mapping operator over the lit colour target.
 *
 * What a Vulkan renderer runs between its lighting pass and the present: the RGBA16F colour target holds unbounded values
 * once lights add up (include/svr_lighting.h), and svr_copy_to_swapchain only clamps them.  This pass scales the target by
 * an exposure, adds a bloom built from a pyramid of blurred half-resolution levels, and maps the sum into [0, 1].
 *
 * In place on the context's colour target, RGBA16F only
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED (there is no HDR left to map).
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half is copied bit for bit.  Depth, IDs, the
 *     attribute planes and every pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: every tap of every stage clamps to the rectangle's edge, and nothing outside it
 *     is read.
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *
 * Arithmetic, fp32; I is the scissor's texel, san(v) = v > 0 ? min(v, 65504) : 0
 *   - levels: extents (w + 1) / 2, (h + 1) / 2 of the one before, starting from the scissor's; an extent of 1 stays 1;
 *   - level 0: the 2 x 2 box of san(I), times exposure, minus bloom_threshold, san again; level i: the box of level i - 1;
 *     each blurred with the separable {1, 4, 6, 4, 1} / 16 kernel (edge clamped) and stored as halves;
 *   - from the smallest level up: level i += the bilinear upsample of level i + 1, stored as halves (at most 65504);
 *   - h = san(bloom_intensity * upsample(level 0) + exposure * I), then the operator:
 *       SVR_TONEMAP_CLAMP     min(h, 1)
 *       SVR_TONEMAP_REINHARD  h / (1 + h)
 *       SVR_TONEMAP_ACES      min(h (2.51 h + 0.03) / (h (2.43 h + 0.59) + 0.14), 1)   (Narkowicz's rational fit)
 *     NaN and negative inputs count as 0, +inf as 65504.
 *
 * Refusals, with nothing changed (SVR_ERR_INVALID_ARGUMENT): null arguments, an exposure that is not finite and greater
 * than 0, a bloom_threshold or bloom_intensity that is not finite and at least 0, bloom_levels above SVR_POST_MAX_LEVELS,
 * an unknown operator.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_light_pass: at most 2 * bloom_levels kernels (one with
 *     no bloom).  While an earlier pass's queue overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs
 *     again, once, in call order behind the replayed passes; a pass that ran before the overflowing one is not run again
 *     (DESIGN.md §5 "Post pass").  The result is that of applying every post pass exactly once.
 *   - A caller-bound colour target must stay valid and unchanged, except by operations of this context, until the next fence.
 *   - Scratch: the level images, owned by the context, sized for its extent and allocated by the first post pass.
 *
 * Out of scope
 *   - Multiview layers, RGBA8 targets, interleaved row ownership.
 *   - The sharded frame (svr_dist.h): a band rank blooms its own rows only, so the bloom has seams at band edges.
 *   - An sRGB or gamma transfer (the swapchain formats are UNORM).
 *
 * Auto-exposure is include/svr_exposure.h: under svr_set_post_auto_exposure this pass multiplies `exposure` by the exposure
 * metered on the device (e = exposure * state.exposure, one fp32 multiply), and `exposure` acts as a compensation.
 *
 * HIP library only: the CPU oracle has no post pass.
 */
#ifndef SVR_POST_H
#define SVR_POST_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_POST_MAX_LEVELS 8
enum { SVR_TONEMAP_CLAMP = 0, SVR_TONEMAP_REINHARD = 1, SVR_TONEMAP_ACES = 2 };

typedef struct SvrPostPass {
  float exposure;        /* finite, > 0 */
  float bloom_threshold; /* finite, >= 0, in exposed units */
  float bloom_intensity; /* finite, >= 0 */
  uint32_t bloom_levels; /* 0 .. SVR_POST_MAX_LEVELS; 0 = no bloom */
  uint32_t tonemap;      /* SVR_TONEMAP_* */
} SvrPostPass; /* 20 bytes */

/* Expose, bloom and tone-map the scissor's pixels of the colour target in place (see above). */
int svr_post_pass(SvrContext* ctx, const SvrPostPass* pass);

#ifdef __cplusplus
}
#endif
#endif /* SVR_POST_H */
