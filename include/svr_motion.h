/* svr_motion.h — the camera motion blur pass: streaks gathered along the reprojected velocity over the HDR colour target.
 *
 * Every other stage of the chain takes an instantaneous snapshot.  This pass gives the camera a shutter: each pixel gets
 * a velocity, in pixels, from its own depth and the matrix the temporal pass reprojects with, and gathers 16 or 32 taps
 * along the dominant velocity near it.  A texel spreads over a pixel as far as its own motion along that direction
 * reaches, and of a pixel and a tap the nearer surface decides: a moving foreground bleeds over a still background and
 * lets it show through, a still foreground in front of a moving background keeps its pixels.  The pass follows the camera
 * only, exactly as svr_temporal_resolve does.
 *
 * In place on the context's colour target, RGBA16F only, in scene-linear units
 *   - Meant to run behind svr_temporal_resolve, so that the history stays sharp and blur does not accumulate in it, and in
 *     front of svr_meter_exposure and svr_post_pass, so that bloom sees the streaks.
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half is copied bit for bit.  Depth, IDs, the
 *     attribute planes and every pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: cells are counted from its origin, every tap and every cell clamps to its
 *     edge, and nothing outside it is read.  The velocity is formed from absolute pixel coordinates and the context's
 *     extent, as the temporal pass forms the history position.
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *   - shutter == 0 or max_blur == 0 leaves every bit of the target as it was: the call validates, enqueues nothing and
 *     returns SVR_OK.
 *   - A depth texel, whatever its bits (NaN among them), only enters arithmetic: every address is formed from clamped
 *     integers, as in the temporal pass.
 *
 * Arithmetic, fp32
 *   - velocity: q = reproject * (xn, yn, depth, 1) and (hx, hy) as svr_temporal.h's history position; hs = 0.5 * shutter;
 *     v = ((px + 0.5 - hx) * hs, (py + 0.5 - hy) * hs); (0, 0) unless q.w > 0 and both are finite; with l =
 *     sqrt(fma(vy, vy, vx * vx)) > max_blur both are multiplied by max_blur / l; both are rounded to fp16.  A cleared pixel
 *     needs no special case;
 *   - prepared image: per scissor pixel the three RGB halves after san (svr_post.h's: NaN and negatives 0, +inf the
 *     largest half), the two velocity halves and the depth's bits;
 *   - cells: 8 x 8 pixels from the scissor's origin, clipped; a texel's key is the 64-bit integer bits(len2) << 32 |
 *     vx_half << 16 | vy_half with len2 = fma(vy, vy, vx * vx) of the stored halves; M(cell) the largest key in it; with
 *     Rc = (ceil(max_blur) + 7) / 8, G is the largest M within +-Rc cells, clamped to the cell grid: its low word is the
 *     cell's dominant velocity (gx, gy), its high word L2.  A cell with L2 < 0.25 leaves as san(input), bit for bit;
 *   - taps: n = L2 > 64 ? 32 : 16; s_j = (2 j + 1) / n; in the order +s_0, -s_0, +s_1, -s_1, ... tap k reads the prepared
 *     texel at (x + rint(gx * s), y + rint(gy * s)), ties to even, clamped to the scissor; D_k = sqrt(dx^2 + dy^2) of the
 *     unclamped offsets; a tap with a zero offset has weight 0 and still counts in n; no offset exceeds ceil(max_blur);
 *   - reach and weight: gl = sqrt(L2), rgl = 1 / gl; e(v) = |fma(v.y, gy, v.x * gx)| * rgl; for tap k, e = z_k < z_p ?
 *     e(v_p) : e(v_k) on the depth texels' values (reversed Z: the nearer surface decides, equal depths take the tap's);
 *     w_k = sat(e - D_k + 1).  There is no quotient per tap;
 *   - sum: acc_c = fma(w_k, I_k, acc_c), S += w_k, k ascending; acc_c = fma(n - S, I_p, acc_c); out = san(acc * (1 / n)),
 *     stored as halves.  S <= n, so the pixel's own colour takes the share of the shutter time no tap claimed.
 *   A pixel none of whose taps has weight leaves as san(input), bit for bit; with reproject the identity every pixel does.
 *
 * Refusals, with nothing changed
 *   - SVR_ERR_INVALID_ARGUMENT: null arguments; a matrix entry or field that is not finite; shutter < 0; max_blur outside
 *     [0, SVR_MOTION_MAX_BLUR].
 *   - SVR_ERR_UNSUPPORTED: an RGBA8 target, a row interleave above 1.  Multiview layers have no entry point here: the
 *     pass works on the context's own targets only.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_dof_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, once, in call order behind the
 *     replayed passes; a pass that ran before the overflowing one is not run again (DESIGN.md §5 "Motion blur").  The
 *     result is that of applying every motion blur pass exactly once.
 *   - A caller-bound colour or depth target must stay valid and unchanged, except by operations of this context, until
 *     the next fence.
 *   - Scratch: the prepared image and the cell image, owned by the context, sized for its extent and allocated by the
 *     first motion blur pass.
 *
 * Out of scope
 *   - The CPU oracle: HIP library only.
 *   - Multiview layers.
 *   - The sharded frame (svr_dist.h): a band rank would clamp its taps and cells at its band's edge.
 *   - Per-object motion: the camera only.  A moving object keeps its sharp pixels.
 *   - Per-pixel dither of the tap positions.
 *   - A direction per tap: the cell's dominant direction is used.
 */
#ifndef SVR_MOTION_H
#define SVR_MOTION_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_MOTION_MAX_BLUR 16

typedef struct SvrMotionBlurPass {
  float reproject[16]; /* column-major, SvrTemporalPass.reproject's definition: prev_viewproj * inverse(viewproj), no jitter */
  float shutter;       /* finite, >= 0: the part of the frame interval the shutter is open; the streak reaches shutter/2 of the motion either way */
  float max_blur;      /* finite, 0 .. SVR_MOTION_MAX_BLUR: no streak reaches farther from its pixel, in pixels */
} SvrMotionBlurPass;   /* 72 bytes */

/* Blur the scissor's pixels of the colour target in place along the camera's motion (see above). */
int svr_motion_blur_pass(SvrContext* ctx, const SvrMotionBlurPass* pass);

#ifdef __cplusplus
}
#endif
#endif /* SVR_MOTION_H */
