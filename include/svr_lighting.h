/* svr_lighting.h — a deferred lighting pass: a shadowed sun and tiled point lights over the G-buffer.
 *
 * What a Vulkan renderer runs after its G-buffer pass: a full-screen compute pass that reads depth, normal and albedo,
 * looks the sun up in a shadow map and adds the point lights that reach the pixel's screen tile.  The inputs are what
 * the other headers produce: the depth target, the SVR_ATTR_NORMAL and SVR_ATTR_ALBEDO planes of a geometry pass
 * (include/svr_attributes.h), and, as the shadow map, the depth target of a depth-only pass drawn from the light
 * (include/svr_depth.h) in another context, or one layer of a multiview depth array (include/svr_views.h).
 *
 * Inputs, taken as bound when the call is enqueued
 *   - the context's depth target, the current SVR_ATTR_NORMAL target and the current SVR_ATTR_ALBEDO target.  If either
 *     plane is missing: SVR_ERR_INVALID_ARGUMENT.
 *   - A pixel is lit iff the w of its albedo texel has the bits 0x3F800000 (1.0f: an opaque fragment won the pixel).
 *
 * Output: the context's colour target, either colour format
 *   - Every pixel the pass owns whose albedo texel says so gets the lit colour with alpha 1; whatever was blended on it
 *     before is replaced.  The pass owns the scissor; under svr_set_row_interleave its tile rows, counted from the
 *     scissor's first row as everywhere else.
 *   - Every other pixel, and every other target (depth, IDs, attribute planes), is untouched.
 *   - A deferred svr_clear_color runs first: this call writes colour.
 *
 * Arithmetic, fp32
 *   - position: p = inv_viewproj * (xn, yn, depth, 1) / w at the pixel centre;
 *   - sun: mesh.frag's term max(n . L, 0.1) with the stored (not normalised) normal, or 0.1 where the shadow map holds a
 *     nearer depth at p (one texel, nearest, no filtering; outside the map or behind its camera: unshadowed); then
 *     albedo * light * sunlight_color.w + albedo * ambient.  With no point lights and no shadow map this is the forward
 *     pass's opaque colour, bit for bit;
 *   - point light i, for d2 = |pl - p|^2 < radius^2 and n . (pl - p) > 0:
 *       += albedo * color_i * (n . (pl - p) / sqrt(d2)) * ((1 - d2 / radius^2)^2 / (d2 + 1)) * intensity, in index order.
 *   - Lights are culled per 32 x 32 tile against the box of the tile's positions; culling never changes a pixel.
 *
 * Refusals, with nothing changed (SVR_ERR_INVALID_ARGUMENT): null arguments, n_lights > SVR_MAX_LIGHTS, lights == NULL
 * with n_lights > 0, a light whose radius is not finite and greater than 0, a shadow map with a zero extent or an extent
 * above 2^24 (16777216) either way: the extents enter the arithmetic as floats and must be exact there.
 *
 * Ordering
 *   - Stream-ordered on the context's stream, and logged like svr_build_depth_pyramid: the light array is copied at
 *     the call; after a queue overflow of an earlier pass (SVR_OPT_QUEUE_CAPS) the lighting pass runs again, in call
 *     order, behind the replayed passes.  While an earlier pass's overflow is pending it writes nothing.
 *   - The shadow map and caller-bound planes and targets must stay valid and unchanged, except by passes of this context
 *     enqueued before the call, until the next fence (svr_sync or a read-back): after a queue overflow the pass runs again
 *     from the same addresses, behind the replayed passes.  A shadow map drawn by another context must be complete
 *     (that context fenced, or its stream ordered before this one's) before the call.
 *
 * Out of scope
 *   - Multiview layers: the pass lights the context's own targets only.
 *   - Exchange in the sharded frame (svr_dist.h): a rank lights its own rows only; nothing is exchanged.
 *   - Transparent objects in the same pass as the G-buffer: the lighting pass replaces what was blended over an opaque
 *     winner.  Draw them behind it under SVR_DEPTH_LOAD instead (include/svr_load.h): they are tested against the
 *     opaque depth and blended over the lit colour, and the planes survive the pass.
 *   - PCF or otherwise filtered shadows: one nearest texel per pixel.
 *   - The C++ harness (host/) calls it with the scene's sun and ambient only (svr_demo --deferred 1): no point lights,
 *     no shadow map.
 *
 * HIP library only: the CPU oracle has no lighting pass.
 */
#ifndef SVR_LIGHTING_H
#define SVR_LIGHTING_H

#include "svr_attributes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_MAX_LIGHTS 4096

typedef struct SvrPointLight {
  float position[3]; /* world space */
  float radius;      /* finite, > 0: the light reaches points nearer than this */
  float color[3];
  float intensity;
} SvrPointLight; /* 32 bytes */

typedef struct SvrLightPass {
  float inv_viewproj[16];      /* column-major: the inverse of the viewproj the G-buffer was drawn with (caller-computed) */
  float ambient_color[4];      /* as in SvrSceneData */
  float sunlight_direction[4];
  float sunlight_color[4];
  const SvrPointLight* lights; /* host array, borrowed for the call; may be NULL with n_lights == 0 */
  uint32_t n_lights;
  const float* shadow_depth;   /* NULL: unshadowed.  Else device memory, shadow_width * shadow_height floats, reversed-Z */
  uint32_t shadow_width, shadow_height; /* 1 .. 2^24 each */
  float shadow_viewproj[16];   /* the viewproj that depth map was drawn with */
  float shadow_bias;           /* added to the pixel's depth in the map before the comparison */
} SvrLightPass;

/* Light the opaque winners of the pixels the pass owns (see above). */
int svr_light_pass(SvrContext* ctx, const SvrLightPass* pass);
/* Fences, then the number of lights each 32 x 32 tile of the last lighting pass kept after culling, row-major over that
 * pass's tile grid (a tile without a lit pixel: 0); capacity counts uint32 words.  *n_tiles = the tiles; counts may be NULL
 * to ask for the count only.  A test hook. */
int svr_debug_read_light_tiles(SvrContext* ctx, uint32_t* counts, size_t capacity, uint32_t* n_tiles);

#ifdef __cplusplus
}
#endif
#endif /* SVR_LIGHTING_H */
