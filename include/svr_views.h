/* svr_views.h — multiview passes: one scene drawn from up to 16 cameras into the layers of array targets.
 *
 * What Vulkan 1.1's VK_KHR_multiview gives a renderer: one render pass whose draws land in every layer of an array
 * attachment, the view's matrices selected by gl_ViewIndex.  The six faces of a cube map or light probe, the two eyes of
 * a stereo pair, the cameras of a rig: one pass instead of one per view, so the fixed costs of a pass (host work, the
 * stage-1 kernel chain, the wait in front of the tile kernel) are paid once, and the tile kernel gets every layer's tiles.
 *
 * Contract
 *   - Bit-exact per layer.  With the context's width W and height H, layer k of the targets (colour, depth and, if
 *     given, IDs) ends up bit for bit as svr_draw_geometry(scenes[k], same arrays) — or svr_draw_list on the same list —
 *     leaves single W x H targets that held layer k's colour before the call (colour LOAD, depth CLEAR 0.0, IDs as in
 *     svr_ids.h).  With clear_rgba, as svr_clear_color(clear_rgba) followed by that pass.  Both colour formats, every
 *     SVR_OPT_* setting.
 *   - Each view culls on its own (is_visible with scenes[k].viewproj); the opaque order is the single pass's (material,
 *     mesh, index) sort, transparent objects are drawn in submission order.
 *   - One UBO: the views differ in view, proj and viewproj only.  ambient_color, sunlight_direction and sunlight_color
 *     must be bitwise equal across scenes, else SVR_ERR_INVALID_ARGUMENT.
 *   - Limits: 1 <= n_views <= SVR_MAX_VIEWS and n_views * ceil(H / 32) <= 512 (the tile rows of the largest target);
 *     otherwise SVR_ERR_INVALID_ARGUMENT.  A narrowed scissor or a row interleave with stride > 1: SVR_ERR_UNSUPPORTED.
 *     The sharded frame (svr_dist.h) has no multiview form.
 *   - The context's own colour, depth and ID targets are not touched.  A deferred svr_clear_color of the context's
 *     target is not taken over: it runs on that target, in call order, before the multiview pass.
 *   - Stream-ordered and logged like every pass: after a queue overflow (SVR_OPT_QUEUE_CAPS) the pass is replayed into
 *     the targets, scenes and list version it was enqueued with.
 *   - Stats: triangle_count, drawcall_count, culled_draws and the fragment, triangle and bin counters are sums over the
 *     views.  svr_debug_read_bins and svr_debug_read_tile_cycles cover every layer's tiles, layer-major;
 *     svr_get_row_costs keeps reporting the last single-view pass.
 *   - Where the per-view cull and draw records are made: svr_draw_geometry_views on the host (one sort, a cull per
 *     view), whatever SVR_OPT_DEVICE_FLATTEN says.  svr_draw_list_views on the device — one workgroup walks the list's
 *     device copy once per view — for lists of up to 4096 objects, unless SVR_OPT_DEVICE_FLATTEN is 2; larger lists on
 *     the host, from the list as it stands.  The frames are the same either way.
 *   - A pass holds the triangles of every view: like a single-view pass it takes fewer than 2^30 in all (counting every
 *     object of a draw list in every view), else SVR_ERR_UNSUPPORTED.
 *   - svr_debug_trace_pixel names a pixel of the context's target: multiview passes record no trace.
 *   - Single-view passes are unchanged: they run the kernels they ran before this header existed.
 *
 * HIP library only: the CPU oracle has no multiview; its svr_draw_geometry, once per view, is the reference.
 */
#ifndef SVR_VIEWS_H
#define SVR_VIEWS_H

#include "svr_draw_list.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVR_MAX_VIEWS 16

typedef struct SvrViewTargets {
  void* color;             /* n_views * W * H texels of the context's colour format: layer-major, each layer row-major
                              with no padding (a tensor [K, H, W, C]); 16-byte aligned */
  float* depth;            /* n_views * W * H floats, same layout, 16-byte aligned */
  uint32_t* ids;           /* NULL, or n_views * W * H * 2 uint32 {object, primitive} as in svr_ids.h, 16-byte aligned */
  const float* clear_rgba; /* NULL: colour LOAD (whatever the caller left there); else every layer pixel starts as this
                              value, encoded exactly as svr_clear_color does */
} SvrViewTargets;

/* svr_draw_geometry for n_views cameras at once: scenes[k] draws layer k.  The arrays are borrowed for the call. */
int svr_draw_geometry_views(SvrContext* ctx, uint32_t n_views, const SvrSceneData* scenes, const SvrViewTargets* targets,
                            const SvrRenderObject* opaque, size_t n_opaque, const SvrRenderObject* transparent,
                            size_t n_transparent, SvrStats* out_stats);
/* svr_draw_list for n_views cameras at once (include/svr_draw_list.h). */
int svr_draw_list_views(SvrContext* ctx, SvrDrawList list, uint32_t n_views, const SvrSceneData* scenes,
                        const SvrViewTargets* targets, SvrStats* out_stats);

#ifdef __cplusplus
}
#endif
#endif /* SVR_VIEWS_H */
