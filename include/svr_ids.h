/* svr_ids.h — the object and primitive ID target: which opaque object and which of its triangles won each pixel.
 *
 * What a Vulkan renderer gets from one more R32G32_UINT colour attachment written by the opaque pipeline: per-pixel
 * picking for click-to-select, hover highlighting and scene debugging.  The tile kernel already resolves every pixel's
 * winning triangle record for shading; with an ID target bound it also writes {object, primitive} out of that record.
 *
 * Layout and meaning
 *   - width * height pixels of two uint32_t each, row-major, no padding: {object, primitive}.
 *   - object: the 1-based position of the winning object in the `opaque` array given to svr_draw_geometry, or in a
 *     draw list's opaque array as created or updated (svr_draw_list.h).
 *   - primitive: the triangle's index within that object's draw, (index position - first_index) / 3, like
 *     gl_PrimitiveID.  Triangles cut by the near plane report their parent triangle.
 *   - {0, 0}: no opaque fragment won the pixel.
 *   - The winner is the fragment whose depth svr_read_depth returns, with its tie rule: the maximum over (depth, key),
 *     so among equal depths the later object in draw order wins.  Transparent objects never write the target (their
 *     depth writes are off too).
 *
 * When it is written
 *   - Every svr_draw_geometry / svr_draw_list pass clears and writes it over the pixels it owns (the scissor; with
 *     svr_set_row_interleave, its tile rows), exactly where it writes depth.  Other pixels are not touched.
 *   - svr_draw_colored_triangle, svr_draw_tex_image, svr_clear_color and svr_draw_background leave it untouched.
 *   - Stream-ordered like the colour and depth targets: a pass writes the ID target bound when it was enqueued, and
 *     so does its replay after a queue overflow (SVR_OPT_QUEUE_CAPS).
 *   - With no ID target, passes run the kernels they ran before this header existed: nothing changes.
 *   - A rank of the sharded frame (svr_dist.h) writes its own rows only; ID rows are not exchanged.
 *
 * HIP library only: the CPU oracle has no ID target.
 */
#ifndef SVR_IDS_H
#define SVR_IDS_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: allocate the context-owned ID plane (zeroed) and make it the ID target unless a caller's target is bound.
 * on == 0: free it (after a fence); if it was the target, there is none from then on. */
int svr_enable_ids(SvrContext* ctx, int on);
/* Caller-owned device memory of width * height * 8 bytes, 16-byte aligned, as the ID target instead of the context's
 * plane (as svr_bind_targets does for colour and depth).  NULL goes back to the context's plane, or to none. */
int svr_bind_id_target(SvrContext* ctx, void* ids_dev);
/* The current ID target's device address; NULL when there is none. */
int svr_get_id_target(SvrContext* ctx, void** ids_dev);
/* Fences, then copies the whole target (width * height * 8 bytes).  No target: SVR_ERR_INVALID_ARGUMENT. */
int svr_read_ids(SvrContext* ctx, uint32_t* dst_host, size_t bytes);
/* Fences, then reads pixel (x, y): out[0] = object, out[1] = primitive.  A pixel outside the target, or no target:
 * SVR_ERR_INVALID_ARGUMENT. */
int svr_pick(SvrContext* ctx, uint32_t x, uint32_t y, uint32_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* SVR_IDS_H */
