/* svr_dof.h — the depth of field pass: a thin-lens blur gathered over the HDR colour target.
 *
 * Every other stage of the chain renders through a pinhole.  This pass gives the camera a lens: each pixel gets a signed
 * blur radius from its depth (negative in front of the focus distance, positive behind it), and gathers 49 taps on a
 * disc as wide as the largest radius near it.  A texel spreads over a pixel as far as its own radius reaches, but a
 * texel behind the pixel no wider than the pixel itself is blurred: an out-of-focus foreground bleeds over a sharp
 * background and not the reverse.
 *
 * In place on the context's colour target, RGBA16F only, in scene-linear units
 *   - Meant to run after svr_fog_pass and before svr_temporal_resolve and svr_post_pass, so that bloom sees the bokeh.
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half is copied bit for bit.  Depth, IDs, the
 *     attribute planes and every pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: cells are counted from its origin, every tap and every cell clamps to its
 *     edge, and nothing outside it is read.
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *   - blur_scale == 0 or max_radius == 0 leaves every bit of the target as it was: the call validates, enqueues nothing
 *     and returns SVR_OK.
 *
 * Arithmetic, fp32
 *   - radius: iz = fma(depth, inv_z_scale, inv_z_bias), r = blur_scale * fma(-focus_distance, iz, 1), a NaN counts as 0,
 *     clamped to [-max_radius, max_radius] and rounded to fp16: the signed radius c.  A cleared pixel (depth bits 0)
 *     needs no special case: iz = inv_z_bias;
 *   - prepared image: per scissor pixel the three RGB halves after san (svr_post.h's: NaN and negatives 0, +inf the
 *     largest half) and c;
 *   - cells: 8 x 8 pixels from the scissor's origin, clipped; M(cell) the largest |c| in it; with R = ceil(max_radius)
 *     and Rc = (R + 7) / 8 the gather radius g of a pixel is the largest M within +-Rc cells of its own, clamped to the
 *     cell grid: the same for the 64 pixels of a cell;
 *   - taps: the centre and three rings of 8, 16 and 24 on the unit disc (the even ring turned by half a step), a table
 *     of fp32 values; tap k reads the prepared texel at (x + rint(u_k.x * g), y + rint(u_k.y * g)), clamped to the
 *     scissor; dist_k = sqrt(dx^2 + dy^2) of the unclamped offsets; a tap k >= 1 with a zero offset has weight 0;
 *   - weight: e_k = c_k > c_p ? min(|c_k|, |c_p|) : |c_k|; w_k = sat(e_k - dist_k + 1) / max(e_k^2, 1);
 *   - sum: acc_c = fma(w_k, I_k, acc_c), W += w_k, k ascending; out = san(acc / W), stored as halves.
 *   A pixel none of whose taps reaches a spreading texel leaves as san(input), bit for bit, and so does every pixel of a
 *   cell with g < 0.5.
 *
 * Refusals, with nothing changed
 *   - SVR_ERR_INVALID_ARGUMENT: null arguments; any field that is not finite; focus_distance <= 0; blur_scale < 0;
 *     max_radius outside [0, SVR_DOF_MAX_RADIUS].
 *   - SVR_ERR_UNSUPPORTED: an RGBA8 target, a row interleave above 1.  Multiview layers have no entry point here: the
 *     pass works on the context's own targets only.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_fog_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, once, in call order behind the
 *     replayed passes; a pass that ran before the overflowing one is not run again (DESIGN.md §5 "Depth of field").
 *     The result is that of applying every depth of field pass exactly once.
 *   - A caller-bound colour or depth target must stay valid and unchanged, except by operations of this context, until
 *     the next fence.
 *   - Scratch: the prepared image and the cell image, owned by the context, sized for its extent and allocated by the
 *     first depth of field pass.
 *
 * Out of scope
 *   - The CPU oracle: HIP library only.
 *   - Multiview layers.
 *   - The sharded frame (svr_dist.h): a band rank blurs its own rows; taps and cells clamp at the band's edge.
 *   - A focus range: one focus distance, and the radius grows on either side of it at once.
 *   - Shaped apertures: the disc only.
 */
#ifndef SVR_DOF_H
#define SVR_DOF_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_DOF_MAX_RADIUS 16

typedef struct SvrDofPass {
  float inv_z_scale, inv_z_bias; /* 1 / view distance = fma(depth, inv_z_scale, inv_z_bias); finite */
  float focus_distance;          /* finite, > 0: the view distance that is sharp */
  float blur_scale;              /* finite, >= 0: the blur radius, in pixels, of a point at infinity */
  float max_radius;              /* finite, 0 .. SVR_DOF_MAX_RADIUS: no radius is larger, either side of focus */
} SvrDofPass; /* 20 bytes */

/* Blur the scissor's pixels of the colour target in place (see above). */
int svr_dof_pass(SvrContext* ctx, const SvrDofPass* pass);

#ifdef __cplusplus
}
#endif
#endif /* SVR_DOF_H */
