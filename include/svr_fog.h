/* svr_fog.h — the fog pass: height fog and sun shafts, marched through the lighting pass's shadow map.
 *
 * What a Vulkan renderer runs between its lighting pass and its post pass: every stage before it treats the space
 * between the camera and the surface as empty.  This pass marches one ray per 2 x 2 block of pixels from the camera to
 * the block's farthest surface through an exponential height fog, looks the sun up in the shadow map at every sample
 * (include/svr_lighting.h's map, read along the ray instead of on the surface), and composites the in-scattered
 * radiance S and the transmittance T over the colour target with a depth-aware upsample: out = I * T + S.
 *
 * In place on the context's colour target, RGBA16F only, in scene-linear units
 *   - Meant to run after svr_light_pass (and the transparents drawn under SVR_DEPTH_LOAD) and before svr_post_pass.
 *   - An RGBA8 target: SVR_ERR_UNSUPPORTED.
 *   - Only the RGB halves of the scissor's pixels are written; the alpha half is copied bit for bit.  Depth, IDs, the
 *     attribute planes and every pixel outside the scissor are untouched.
 *   - The scissor rectangle is the image: the half-resolution grid covers it, every tap clamps to the grid's edge, and
 *     nothing outside it is read.
 *   - Under svr_set_row_interleave with a stride above 1: SVR_ERR_UNSUPPORTED.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *   - density == 0 leaves every bit of the target as it was: the call validates, enqueues nothing and returns SVR_OK.
 *
 * Arithmetic, fp32
 *   - grid: (w + 1) / 2 by (h + 1) / 2 blocks over the scissor; block (bx, by) covers its pixels 2bx .. 2bx + 1,
 *     2by .. 2by + 1, clipped.  One ray per block, from camera_position through the block's centre unprojected at
 *     depth 1 (the near plane), of length t_end = the largest t(pixel) of the block, t(pixel) = min(|p - camera|,
 *     max_distance) with p the pixel's position (C17); a pixel whose depth bits are 0 (the clear value) has
 *     t = max_distance;
 *   - march: delta = t_end / steps, sample i at t_i = (i + o) * delta with o = the top 8 bits of an integer hash of
 *     (bx, by, frame_index) over 256; extinction sigma_i = density * 2^(-height_falloff * log2(e) * (y_i - height_base)),
 *     step transmittance a_i = 2^(-sigma_i * delta * log2(e)), both through C41's polynomial with the argument clamped
 *     to its range (so a_i >= 2^-16 per step); v_i = C18's shadow lookup at the sample (outside the map or behind its
 *     camera: lit); phase ph = (1 - g^2) / (4 pi x sqrt(x)), x = 1 + g^2 - 2 g (dir . L / |L|), once per ray;
 *       S += T (1 - a_i) (fog_color + sun_color v_i ph), then T *= a_i, from S = 0, T = 1;
 *   - composite: the four half-resolution taps around the pixel, bilinear weights b_k divided by
 *     1 + edge_sharpness |t_end_k - t(pixel)|, normalised; out = san(I * T + S), san as in svr_post.h.
 *
 * Refusals, with nothing changed
 *   - SVR_ERR_INVALID_ARGUMENT: null arguments; a density, height_falloff or edge_sharpness that is not finite and at
 *     least 0; a max_distance that is not finite and greater than 0; steps outside 1 .. SVR_FOG_MAX_STEPS; an anisotropy
 *     that is not |g| < 1; a shadow map with a zero extent or an extent above 2^24 either way (the lighting pass's rule).
 *   - SVR_ERR_UNSUPPORTED: an RGBA8 target, a row interleave above 1.  Multiview layers have no entry point here: the
 *     pass works on the context's own targets only.
 *
 * Ordering
 *   - Stream-ordered on the context's stream and logged like svr_post_pass: two kernels.  While an earlier pass's queue
 *     overflow is pending (SVR_OPT_QUEUE_CAPS) the pass writes nothing and runs again, once, in call order behind the
 *     replayed passes; a pass that ran before the overflowing one is not run again (DESIGN.md §5 "Fog pass").  The
 *     result is that of applying every fog pass exactly once.
 *   - The shadow map and a caller-bound colour or depth target must stay valid and unchanged, except by operations of
 *     this context, until the next fence.
 *   - Scratch: the half-resolution images (S, T and t_end per block), owned by the context, sized for its extent and
 *     allocated by the first fog pass.
 *
 * Out of scope
 *   - The CPU oracle: HIP library only.
 *   - Point lights scattering in the medium: the sun and the ambient fog_color only.
 *   - The sharded frame (svr_dist.h): a band rank fogs its own rows; the upsample's taps clamp at the band's edge.
 *   - Cascades or filtered shadows: one map, one nearest texel per sample.
 */
#ifndef SVR_FOG_H
#define SVR_FOG_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_FOG_MAX_STEPS 64

typedef struct SvrFogPass {
  float inv_viewproj[16];      /* column-major: the inverse of the viewproj the depth target was drawn with */
  float camera_position[3];    /* world space: where every ray starts */
  float density;               /* finite, >= 0: the extinction at height_base, per world unit */
  float height_falloff;        /* finite, >= 0; 0: uniform fog */
  float height_base;           /* world y */
  float max_distance;          /* finite, > 0: no ray is marched farther */
  uint32_t steps;              /* 1 .. SVR_FOG_MAX_STEPS samples per ray */
  float fog_color[3];          /* ambient in-scattered radiance */
  float anisotropy;            /* Henyey-Greenstein g, |g| < 1 */
  float sunlight_direction[4]; /* towards the sun, as in SvrSceneData; xyz are normalised by the pass */
  float sun_color[3];
  float edge_sharpness;        /* finite, >= 0: how fast a tap at another distance loses weight; 0: plain bilinear */
  const float* shadow_depth;   /* NULL: unshadowed.  Else as in SvrLightPass */
  uint32_t shadow_width, shadow_height; /* 1 .. 2^24 each */
  float shadow_viewproj[16];
  float shadow_bias;
  uint32_t frame_index;        /* seeds the dither */
} SvrFogPass; /* 232 bytes */

/* Fog the scissor's pixels of the colour target in place (see above). */
int svr_fog_pass(SvrContext* ctx, const SvrFogPass* pass);

#ifdef __cplusplus
}
#endif
#endif /* SVR_FOG_H */
