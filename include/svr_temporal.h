/* svr_temporal.h — temporal antialiasing: jittered frames resolved against a reprojected, clamped history.
 *
 * Coverage in this library is one exact sample per pixel centre.  The caller shifts the projection by a sub-pixel jitter
 * each frame (Scene.viewproj is caller-supplied; host/svr_math.h jitter_projection, halton), and this pass blends the
 * frame with last frame's resolved colour: the history is fetched where the pixel's surface was last frame (through the
 * depth target and one matrix), clamped to the range of the current 3 x 3 neighbourhood, and mixed in.
 *
 * In place on the context's colour target, RGBA16F only
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half, depth, IDs, the attribute planes and every
 *     pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: every tap of colour, depth and history clamps to the rectangle's edge, and
 *     nothing outside it is read.
 *   - The depth target is read as it stands in stream order.  Its texels must not be NaN (else the pixels are unspecified;
 *     never a fault: a depth is arithmetic only, every address comes from clamped integers or tested floats).
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *
 * History
 *   - Two RGBA16F images owned by the context, sized for its extent, allocated by the first resolve.  A resolve reads one
 *     and writes the other; the next resolve reads what this one wrote.
 *   - The history is valid iff an earlier resolve of this context was accepted, that resolve had the same scissor
 *     rectangle, and this call does not carry SVR_TEMPORAL_RESET.  Otherwise every pixel takes the current colour.
 *   - Validity and the two roles are decided at the call, in call order, and travel with the logged operation by value.
 *
 * Arithmetic, fp32; I is the colour texel, san(v) = v > 0 ? min(v, 65504) : 0; W, H the extent
 *   - c = san(I); mn, mx its per-channel minimum and maximum over the 3 x 3 texels around the pixel; z the largest depth of
 *     the same 3 x 3 (reversed-Z: the nearest surface);
 *   - q = reproject * (xn, yn, z, 1) with xn = (px + 0.5) 2/W - 1; the history is invalid for the pixel unless q.w > 0 and
 *     hx = (q.x / q.w) W/2 + W/2, hy likewise, fall inside the scissor;
 *   - hist = the bilinear sample of the history at (hx - 0.5, hy - 0.5); clamped into [mn, mx] unless SVR_TEMPORAL_NO_CLAMP;
 *   - o = hist + blend (c - hist), or c where the history is invalid or blend is 1; stored as halves to the new history
 *     (fourth half 0) and, the same bits, to the colour target's RGB halves.
 *
 * Refusals, with nothing changed, history state included: SVR_ERR_INVALID_ARGUMENT for null arguments, a blend that is
 * not finite or outside (0, 1], unknown flag bits, a non-finite reproject entry.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_post_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, once, in call order behind the
 *     replayed passes, with the history roles it was given at the call; a pass that ran before the overflowing one is not
 *     run again (DESIGN.md §5 "Temporal antialiasing").
 *   - A caller-bound colour or depth target must stay valid and unchanged, except by operations of this context, until the
 *     next fence.
 *
 * Cost: see DESIGN.md §5 "Temporal antialiasing".
 *
 * Out of scope
 *   - Multiview layers, RGBA8 targets, interleaved row ownership.
 *   - The sharded frame (svr_dist.h): a band rank would clamp taps at its band's edge and keep its own history.
 *   - Per-object motion vectors: reprojection follows the camera only; moving objects are held by the neighbourhood clamp.
 *   - Variance clipping, sharpening, a YCoCg neighbourhood.
 *
 * HIP library only: the CPU oracle has no temporal pass.
 */
#ifndef SVR_TEMPORAL_H
#define SVR_TEMPORAL_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SVR_TEMPORAL_RESET = 1u, SVR_TEMPORAL_NO_CLAMP = 2u };

typedef struct SvrTemporalPass {
  float reproject[16]; /* column-major: prev_viewproj * inverse(viewproj), both WITHOUT jitter, caller-computed */
  float blend;         /* weight of the current frame: finite, 0 < blend <= 1 */
  uint32_t flags;      /* SVR_TEMPORAL_* */
} SvrTemporalPass;     /* 72 bytes */

/* Resolve the scissor's pixels of the colour target against the history, in place (see above). */
int svr_temporal_resolve(SvrContext* ctx, const SvrTemporalPass* pass);

/* Test hook: fences, then copies the history the next resolve will read, as RGBA halves over the context's extent
 * (width * height * 8 bytes; zeros before the first resolve).  *valid: 1 iff a resolve with the current scissor and
 * without SVR_TEMPORAL_RESET would use it.  dst may be null to query *valid alone. */
int svr_debug_read_temporal_history(SvrContext* ctx, void* dst, size_t bytes, uint32_t* valid);

#ifdef __cplusplus
}
#endif
#endif /* SVR_TEMPORAL_H */
