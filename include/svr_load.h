/* svr_load.h — the depth loadOp: draw a pass over the depth the target already holds.
 *
 * Every geometry pass begins with depth CLEAR 0.0 (reversed-Z: the far plane).  With SVR_DEPTH_LOAD set a pass begins
 * from the depth target as it stands instead: what a Vulkan renderer gets from loadOp = LOAD on its depth attachment.
 * It is what lets a frame be drawn in more than one pass:
 *   - transparent objects over a deferred frame: opaque pass with planes, svr_light_pass (include/svr_lighting.h), then
 *     the transparent objects under LOAD, tested against the opaque depth and blended over the lit colour;
 *   - a forward overlay over a finished frame, or objects that arrive in groups;
 *   - drawing over a depth image the caller produced and bound with svr_bind_targets.
 *
 * State, like svr_set_scissor: the op holds for every later call until it is set again, and a call takes it as set when
 * the call is enqueued.  The default is SVR_DEPTH_CLEAR.
 *
 * Which calls load
 *   - svr_draw_geometry and svr_draw_list (single view).  The loaded depth is the depth target as it stands when the pass
 *     runs in stream order, over the pixels the pass owns: the scissor, and under svr_set_row_interleave its tile rows.
 *     Both colour formats, every SVR_OPT_* setting.
 *   - svr_draw_colored_triangle and svr_draw_tex_image keep clearing, whatever the op.
 *   - Refused with SVR_ERR_UNSUPPORTED and nothing changed while SVR_DEPTH_LOAD is set: the multiview calls
 *     (svr_draw_geometry_views, svr_draw_list_views, svr_draw_depth_views, svr_draw_list_depth_views) and the depth-only
 *     calls (svr_draw_depth, svr_draw_list_depth).
 *
 * What a LOAD pass computes
 *   - Depth test: an opaque fragment wins its pixel iff its depth bits are greater than or equal to the loaded bits (and it
 *     wins among the pass's own fragments as always: the largest (depth, submission key)).  GREATER_OR_EQUAL against the
 *     loaded depth: at equal depth the pass wins.
 *   - Transparent fragments test against the pass's final depth — loaded, or raised by this pass's opaque winners — and do
 *     not write it.
 *   - A pixel no fragment wins keeps its depth.  Its colour is LOAD, as in every pass, and a deferred svr_clear_color
 *     still lands in it.
 *   - Depth written: the elementwise maximum of loaded and drawn depth, as bit patterns.  Loaded values must be floats in
 *     [0, 1]; anything else gives unspecified pixels but never a fault (the loaded depth never forms an address).
 *   - The hierarchical depth test starts from the loaded depth and may drop triangles it hides; no pixel changes by that.
 *   - A bound occlusion pyramid stays legal under the condition include/svr_occlusion.h states: the pyramid is at or behind
 *     the pass's FINAL depth — which the loaded depth is part of.
 *   - The ID target and the attribute planes are left untouched by a LOAD pass, bound or not (as svr_draw_tex_image leaves
 *     them): the G-buffer survives the pass drawn over it.  Opaque winners of a LOAD pass therefore do not appear in the
 *     IDs or the planes.
 *   - SvrStats, svr_get_row_costs and svr_debug_read_bins report as for a CLEAR pass of the same objects.
 *
 * Ordering: a LOAD pass is logged and replayed like any pass.  A pass that overflowed a queue (SVR_OPT_QUEUE_CAPS) wrote
 * nothing, and neither did anything behind it; the replay runs them again in call order, so a replayed LOAD pass loads the
 * depth the replayed passes before it have just written.  A caller-bound depth image must stay valid and unchanged,
 * except by passes of this context, until the next fence.
 *
 * Out of scope: LOAD for depth-only and multiview passes; IDs and planes updated by a LOAD pass.
 *
 * HIP library only: the CPU oracle always clears.
 */
#ifndef SVR_LOAD_H
#define SVR_LOAD_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum SvrDepthLoadOp { SVR_DEPTH_CLEAR = 0, SVR_DEPTH_LOAD = 1 };

/* The depth loadOp of later geometry passes (see above).  Another value: SVR_ERR_INVALID_ARGUMENT, nothing changed. */
int svr_set_depth_load_op(SvrContext* ctx, int op);
int svr_get_depth_load_op(SvrContext* ctx, int* op);

#ifdef __cplusplus
}
#endif
#endif /* SVR_LOAD_H */
