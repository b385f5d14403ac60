/* svr_occlusion.h — occlusion culling: whole wave chunks of triangles dropped against a min-depth pyramid.
 *
 * What a GPU-driven Vulkan renderer does with a depth pyramid (a "Hi-Z" buffer): before a chunk of triangles is set
 * up, binned and rasterised, the nearest depth it can reach is compared with the farthest depth already known over its
 * screen rectangle; a chunk that is behind everywhere goes no further.  The depth comes from the caller: a depth-only
 * pass of a few large occluders (svr_draw_depth / svr_draw_list_depth, include/svr_depth.h), or the previous frame's
 * depth target with the same camera.
 *
 * Pyramid
 *   - Sized for the context's W x H.  Level l >= 1 has ceil(W / 2^l) x ceil(H / 2^l) texels, down to the first level
 *     that is 1 x 1 (a 1 x 1 context has one level, l = 1).  Level 0 is the depth target itself and is not stored.
 *   - Texel (x, y) of level l is the minimum, taken over the uint32 bit patterns, of the depth pixels in
 *     [x 2^l, (x + 1) 2^l) x [y 2^l, (y + 1) 2^l) that lie inside the frame.  Depth is reversed-Z (cleared to 0.0, nearer
 *     is larger), so this is the farthest depth there.  Bit patterns, because the depth test orders depth that way
 *     (a maximum over (depth bits, key)): +-0 and NaNs need no rule of their own.
 *   - svr_build_depth_pyramid is stream-ordered on the context's stream, and logged like a clear: after a queue
 *     overflow (SVR_OPT_QUEUE_CAPS) it runs again, in call order, after the passes in front of it have been replayed,
 *     so it reads the replayed depth.  While an earlier pass's overflow is pending it writes nothing.
 *
 * Culling
 *   - svr_set_occlusion_pyramid(ctx, pyr): every later single-view pass culls against pyr as it stands when the pass
 *     runs — svr_draw_geometry (host or device flatten), svr_draw_list, svr_draw_depth and svr_draw_list_depth, either
 *     colour format, with a scissor, a row interleave, an ID target, SVR_OPT_COUNT_FRAGMENTS or not.  A pass's culling
 *     waits for the last svr_build_depth_pyramid of its pyramid enqueued before it.  0 switches culling off; with no
 *     pyramid bound the passes run exactly as without this header.
 *   - A wave chunk (64 triangles of one draw, the unit of the setup kernel) is culled only if
 *       (a) all eight corners of its object-space box (the mesh's index-group table) are finite in clip space, with
 *           w > 0, 0 <= z <= w (in front of the far plane, on the inner side of the near plane), and
 *       (b) a float bound on the largest depth any of its fragments can reach, margins included, is
 *           strictly below, as bit patterns, the minimum of the pyramid texels that cover its rectangle: the corners'
 *           screen image, widened by one pixel and clamped to the scissor.
 *     Level rule: the smallest l >= 1 at which the rectangle spans at most 4 x 4 texels (the top level if none does);
 *     sixteen lanes read one texel each.  Boxes with a non-finite vertex behind them are never culled.
 *   - Culled triangles are not clipped, binned or rasterised.  triangle_count, drawcall_count, culled_draws and
 *     shaded_fragments are those of the pass without culling; rasterized_fragments, binned_triangles and bin_entries
 *     count what survives.
 *
 * The guarantee
 *   Suppose every texel of the pyramid is at or behind, as bit patterns, the depth the same pass without culling would
 *   leave on every pixel the texel covers and the pass owns (inside the scissor, on the pass's tile rows).  Then the
 *   pass leaves colour, depth and ID targets bit for bit as the pass without culling.  Why: the tile kernel's fragment
 *   depth is clamped to [0, 1], where bit order is float order, so every fragment of a culled chunk is strictly below
 *   the bound, which is strictly below every texel over its pixel, which is at or below that pixel's final depth.  The
 *   final depth and ID are a maximum over (depth bits, key) of the pass's opaque fragments, so a fragment strictly
 *   behind it wins no pixel and ties with none: dropping it changes neither.  Transparent fragments behind the final
 *   opaque depth fail the depth test, so dropping them changes no colour either.
 *   The two usual ways to meet the condition: a depth-only pass of a subset of the opaque objects with the same camera
 *   and scissor, then a build; or the depth the same pass left last frame, with the same camera and list.
 *
 * Limits
 *   - Multiview passes (include/svr_views.h, svr_draw_*_views) with a pyramid bound return SVR_ERR_UNSUPPORTED.
 *   - The sharded frame (svr_dist.h, dist.py) does not cull.
 *   - Handles are 1-based; 0 is no pyramid.
 *
 * Stats
 *   svr_get_occlusion_stats reports the chunks that reached the occlusion test, the chunks culled and their triangles,
 *   like the fragment counters of SvrStats: of the last pass run with SVR_OPT_COUNT_FRAGMENTS (uninstrumented passes
 *   report nothing).  svr_debug_read_occlusion has one bit per chunk of the last pass, instrumented or not.
 *
 * HIP library only: the CPU oracle has no pyramid.
 */
#ifndef SVR_OCCLUSION_H
#define SVR_OCCLUSION_H

#include "svr_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef uint32_t SvrDepthPyramid;

typedef struct SvrOcclusionStats {
  uint64_t chunks_tested;    /* wave chunks that reached the occlusion test (inside the frustum, finite box) */
  uint64_t chunks_culled;    /* ... of them culled */
  uint64_t triangles_culled; /* the triangles of the culled chunks */
} SvrOcclusionStats;

/* A pyramid for the context's extent.  *out = its handle. */
int svr_create_depth_pyramid(SvrContext* ctx, SvrDepthPyramid* out);
/* The handle goes at once (and, if it was bound for culling, is unbound); the memory after the last operation that
 * uses it. */
int svr_destroy_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr);
/* Build pyr from a W x H float depth target on the device: NULL = the context's depth target as bound now.  A caller's
 * buffer (for example layer k of a multiview depth array; 16-byte aligned reads fastest) must stay valid and unchanged,
 * except by passes of this context enqueued before the build, until the next fence (svr_sync or a read-back): after a
 * queue overflow the build runs again from the same address, behind the replayed passes. */
int svr_build_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr, const float* depth_dev);
/* Later passes cull against pyr; 0 = no culling. */
int svr_set_occlusion_pyramid(SvrContext* ctx, SvrDepthPyramid pyr);
/* Fences, then copies level (1 ..) of pyr to dst: ceil(W / 2^level) * ceil(H / 2^level) uint32 bit patterns, row-major.
 * *n_levels (if not NULL) = the pyramid's levels.  A test hook. */
int svr_read_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr, uint32_t level, void* dst, size_t bytes, uint32_t* n_levels);
/* The occlusion counters (see Stats above). */
int svr_get_occlusion_stats(SvrContext* ctx, SvrOcclusionStats* out);
/* Fences, then one bit per wave chunk of the last pass, in the order of svr_debug_read_records' chunks: bit i % 32 of
 * bits[i / 32] is 1 if chunk i was culled; capacity counts uint32 words.  *n_chunks = the chunks; bits may be NULL to ask
 * for the count only. */
int svr_debug_read_occlusion(SvrContext* ctx, uint32_t* bits, size_t capacity, uint32_t* n_chunks);

#ifdef __cplusplus
}
#endif
#endif /* SVR_OCCLUSION_H */
