/* svr_reflect.h — the reflection pass: screen-space rays marched through the depth target.
 *
 * What a deferred Vulkan renderer runs between its lighting pass and its fog: every stage before it lights a pixel from
 * the sun, the point lights and the ambient term only, and no pixel sees another.  This pass reflects the view ray of
 * every opaque pixel about its G-buffer normal, marches the reflected ray through the depth target in equal world-space
 * steps until it passes behind a surface no thicker than `thickness`, bisects the last step, and blends the colour
 * found there over the pixel with a Schlick weight: out = I (1 - k) + k R.
 *
 * In place on the context's colour target, RGBA16F only, in scene-linear units
 *   - Meant to run after svr_light_pass (and the transparents drawn under SVR_DEPTH_LOAD) and before svr_fog_pass.
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half is copied bit for bit.  Depth, IDs, the
 *     attribute planes and every pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: a ray that leaves it misses, every resolve tap clamps to its edge, and
 *     nothing outside it is read.
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - Needs the SVR_ATTR_NORMAL and SVR_ATTR_ALBEDO planes, as the lighting pass does.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *   - intensity == 0 leaves every bit of the target as it was: the call validates, enqueues nothing and returns SVR_OK.
 *
 * Arithmetic, fp32
 *   - which pixels trace (C73): the albedo texel's w is 1.0f bit for bit (an opaque winner), the depth bits are not 0,
 *     and the stored normal has a length; every other pixel has the trace texel 0;
 *   - ray (C74): p = the pixel's position (C17), n^ and v^ = (p - camera) normalised with rcp_ieee(sqrt(.)),
 *     d = n^ . v^, r = v^ - 2 d n^ (not renormalised); h0 = viewproj (p, 1), dh = viewproj (r, 0);
 *   - march (C75): delta = max_distance / steps; sample i = 1 .. steps at t_i = (i + o) delta, o = the top 8 bits of
 *     C56's hash of (x, y, frame_index) over 256; h = h0 + t dh; a sample with h.w <= 0 or whose pixel
 *     floor(h.xy / h.w scaled to the target) is not in the scissor is outside and ends the march as a miss;
 *     q = h.w (depth inv_z_scale + inv_z_bias) of that pixel; behind: q >= 1; hit: 1 <= q <= 1 + thickness; a sample
 *     behind but no hit is passed;
 *   - refinement (C76): `refine` bisections of [t_i - delta, t_i], towards the first sample that is behind;
 *   - weight (C77): k = sat(intensity F fd fe), F = f0 + (1 - f0)(1 - sat(-d))^5, fd = 1 - distance_fade t_hit /
 *     max_distance, fe = the hit pixel's distance to the scissor's border over edge_width; the trace texel is
 *     (k R, k), R = san(rgb) of the hit pixel;
 *   - resolve (C78): the pixel's own trace texel, or the mean of the 3 x 3 taps whose 1 / view distance differs from the
 *     pixel's by at most depth_tolerance times the pixel's;
 *   - composite (C79): out = san(acc.rgb / n + I (1 - acc.w / n)), I = san(input rgb).
 *
 * Refusals, with nothing changed
 *   - SVR_ERR_INVALID_ARGUMENT: null arguments; any float of the pass that is not finite; max_distance not greater
 *     than 0; steps outside 1 .. SVR_REFLECT_MAX_STEPS; refine above SVR_REFLECT_MAX_REFINE; a negative thickness,
 *     intensity, edge_width or depth_tolerance; f0 or distance_fade outside 0 .. 1; resolve above 1; a missing normal
 *     or albedo plane.
 *   - SVR_ERR_UNSUPPORTED: an RGBA8 target, a row interleave above 1.  Multiview layers have no entry point here: the
 *     pass works on the context's own targets only.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_fog_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, once, in call order behind the
 *     replayed passes; a pass that ran before the overflowing one is not run again (DESIGN.md §5 "Reflection pass").
 *     The result is that of applying every reflection pass exactly once.
 *   - A caller-bound colour, depth or attribute target must stay valid and unchanged, except by operations of this
 *     context, until the next fence.
 *   - Scratch: the trace texels (16 bytes per pixel) and a word per 8 x 8 cell, owned by the context, sized for its
 *     extent and allocated by the first reflection pass.
 *
 * Out of scope
 *   - The CPU oracle: HIP library only.
 *   - Multiview layers.
 *   - The sharded frame (svr_dist.h): a band rank reflects what its own rows hold.
 *   - Rays skipped through a depth hierarchy: the pyramid of svr_occlusion.h holds the farthest depth of each cell,
 *     which is what culling needs; a ray skip needs the nearest.  This is a linear march with a bisection refinement.
 *   - Per-material roughness or reflectance: the G-buffer has no such plane, and one f0 serves the frame.
 *   - Rejecting hits on back faces.
 *   - Anything a ray finds off screen or behind the visible surface.
 */
#ifndef SVR_REFLECT_H
#define SVR_REFLECT_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_REFLECT_MAX_STEPS 64
#define SVR_REFLECT_MAX_REFINE 8

typedef struct SvrReflectPass {
  float viewproj[16];       /* column-major: what the G-buffer was drawn with */
  float inv_viewproj[16];   /* its inverse (caller-computed, not checked) */
  float camera_position[3];
  float inv_z_scale, inv_z_bias; /* as in SvrDofPass */
  float max_distance;       /* finite, > 0: world units a ray is marched */
  uint32_t steps;           /* 1 .. SVR_REFLECT_MAX_STEPS */
  uint32_t refine;          /* 0 .. SVR_REFLECT_MAX_REFINE bisections after the first hit */
  float thickness;          /* finite, >= 0: a surface is this thick, relative to its view distance */
  float f0;                 /* 0 .. 1: reflectance at normal incidence */
  float intensity;          /* finite, >= 0 */
  float distance_fade;      /* 0 .. 1: how much of the weight is gone at max_distance */
  float edge_width;         /* finite, >= 0, pixels: hits nearer the scissor's border fade; 0: none */
  uint32_t resolve;         /* 0: one tap; 1: 3 x 3 depth-aware resolve */
  float depth_tolerance;    /* finite, >= 0: relative 1/z difference a resolve tap may have */
  uint32_t frame_index;     /* seeds the dither */
} SvrReflectPass;           /* 192 bytes */

/* Reflect the scissor's pixels of the colour target in place (see above). */
int svr_reflect_pass(SvrContext* ctx, const SvrReflectPass* pass);

#ifdef __cplusplus
}
#endif
#endif /* SVR_REFLECT_H */
