/* svr_depth.h — depth-only passes: the depth target, and the ID target if one is bound, drawn without shading.
 *
 * What a Vulkan render pass with a depth attachment and no colour attachment (colorAttachmentCount = 0) gives a renderer:
 * shadow maps, cube depth maps, depth maps for a sensor model or a dataset, picking-only and segmentation frames.  The
 * tile kernel's depth target is final at the end of its visibility phase, and the ID target leaves with it; a depth-only
 * pass runs that phase and that store, and no fragment stage, transparent layers or colour write-back.  Its setup stage
 * computes gl_Position only and writes only the part of each triangle record the visibility phase reads.
 *
 * Contract
 *   - Targets.  svr_draw_depth leaves the context's depth target, and its ID target if one is bound (svr_ids.h), bit for
 *     bit as svr_draw_geometry(ctx, scene, opaque, n_opaque, NULL, 0) would.  svr_draw_list_depth leaves them as
 *     svr_draw_list would, with the list's transparent objects ignored (transparent objects never write depth or IDs).
 *     Both colour formats, the scissor, svr_set_row_interleave and every SVR_OPT_* setting (SVR_OPT_TUNING bits 5/6
 *     included).  Pixels outside the rows the pass owns are not touched, as with a colour pass.
 *   - Colour.  The colour target is never read or written.  A deferred svr_clear_color stays deferred: it belongs to the
 *     colour target and rides in the next colour pass, or runs when some other call touches colour.  A depth-only pass
 *     neither takes it in nor flushes it.
 *   - Scene data.  Only viewproj is read (the cull and gl_Position); the lighting fields are ignored.
 *   - Multiview.  svr_draw_depth_views / svr_draw_list_depth_views: layer k of targets->depth (and of targets->ids if
 *     given) is what svr_draw_depth(scenes[k]) / svr_draw_list_depth leaves in single W x H targets.  targets->color and
 *     targets->clear_rgba must be NULL, else SVR_ERR_INVALID_ARGUMENT.  The scenes' lighting need not be equal.  The
 *     view count, tile-row limit, narrowed-scissor and interleave refusals are those of svr_views.h.
 *   - Stats.  Those of the equivalent opaque-only svr_draw_geometry pass, field by field (triangle_count, drawcall_count,
 *     culled_draws, rasterized_fragments, binned_triangles, bin_entries), summed over the views of a multiview pass;
 *     shaded_fragments is 0.  As for colour passes, the device-flattened and draw-list forms report their counts through
 *     svr_get_stats after the pass.
 *   - Ordering and replay.  Stream-ordered and logged like every pass: after a queue overflow (SVR_OPT_QUEUE_CAPS) the
 *     pass is replayed into the depth and ID targets it was enqueued with, from the list version it was enqueued with.
 *   - Debug hooks.  svr_get_row_costs keeps reporting the last colour pass.  svr_debug_read_bins and
 *     svr_debug_read_tile_cycles cover the depth-only pass (its transparent bins are empty; phases B to D take 0 cycles).
 *     svr_debug_trace_pixel records nothing: there is no fragment stage.
 *   - The sharded frame (svr_dist.h) has no depth-only form; a depth target of another size than the context's needs a
 *     context of that size.
 *   - Colour passes are unchanged: they run the kernels they ran before this header existed.
 *
 * HIP library only: the CPU oracle has no depth-only pass; its svr_draw_geometry over the opaque objects is the reference.
 */
#ifndef SVR_DEPTH_H
#define SVR_DEPTH_H

#include "svr_views.h"

#ifdef __cplusplus
extern "C" {
#endif

/* svr_draw_geometry(ctx, scene, opaque, n_opaque, NULL, 0), depth and IDs only.  The array is borrowed for the call. */
int svr_draw_depth(SvrContext* ctx, const SvrSceneData* scene, const SvrRenderObject* opaque, size_t n_opaque,
                   SvrStats* out_stats);
/* svr_draw_list over the list's opaque objects (include/svr_draw_list.h), depth and IDs only. */
int svr_draw_list_depth(SvrContext* ctx, SvrDrawList list, const SvrSceneData* scene, SvrStats* out_stats);
/* svr_draw_depth for n_views cameras at once into layered targets (include/svr_views.h); color and clear_rgba NULL. */
int svr_draw_depth_views(SvrContext* ctx, uint32_t n_views, const SvrSceneData* scenes, const SvrViewTargets* targets,
                         const SvrRenderObject* opaque, size_t n_opaque, SvrStats* out_stats);
/* svr_draw_list_depth for n_views cameras at once. */
int svr_draw_list_depth_views(SvrContext* ctx, SvrDrawList list, uint32_t n_views, const SvrSceneData* scenes,
                              const SvrViewTargets* targets, SvrStats* out_stats);

#ifdef __cplusplus
}
#endif
#endif /* SVR_DEPTH_H */
