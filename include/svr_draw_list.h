/* svr_draw_list.h — retained draw lists: a RenderObject list kept in device memory and drawn per frame.
 *
 * The reference rebuilds _main_draw_context in update_scene() every frame (src/vk_engine.cpp:1479-1512) and
 * draw_geometry culls, sorts and records it again (:1357-1477), although between frames only the camera changes.
 * A draw list is that list recorded once: svr_create_draw_list validates the objects, sorts the opaque ones by
 * (material, mesh, submission index) — a key that does not depend on the camera — and copies them into device
 * memory; svr_draw_list then runs the pass of svr_draw_geometry with cull, rank and draw records done by one
 * device kernel (k_flatten.hip list_kernel), with no per-object work on the host.
 *
 * Contract
 *   - svr_draw_list(ctx, L, scene, st) gives the colour target, depth target and stats of
 *     svr_draw_geometry(ctx, scene, <the arrays L holds>) bit for bit, in every state the context can be in
 *     (scissor, row interleave, deferred clear, present status, SVR_OPT_* options).
 *   - Stats: drawcall_count, triangle_count and culled_draws are known after the pass only: out_stats holds 0
 *     there (and mesh_draw_time), svr_get_stats has them — as for svr_draw_geometry's device flatten.
 *   - Updates and destruction are stream-ordered.  A list has versions: svr_update_draw_list makes a new device
 *     copy (copy-on-write) and every pass holds the version it was enqueued with until it has been validated, so
 *     passes in flight — and their replays after a queue overflow (SVR_OPT_QUEUE_CAPS) — see the list as it stood
 *     when they were enqueued.  svr_destroy_draw_list drops the handle at once; the memory goes with its last pass.
 *   - The list names meshes and materials by handle.  Destroying a mesh it names invalidates it: svr_draw_list
 *     then fails with SVR_ERR_INVALID_ARGUMENT (svr_update_draw_list can repair it).  Materials cannot be
 *     destroyed or change pass in this ABI; their colour factors are read from the material table at every pass.
 *   - A list holds at most 16384 objects (the device flatten's bound).
 *   - HIP library only: the CPU oracle has no draw lists; its svr_draw_geometry on the same arrays is the
 *     reference.  Handles are 1-based, 0 is never valid.
 */
#ifndef SVR_DRAW_LIST_H
#define SVR_DRAW_LIST_H

#include "svr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef uint32_t SvrDrawList;

/* Validates every object with svr_draw_geometry's rules (SVR_ERR_BAD_HANDLE / SVR_ERR_INVALID_ARGUMENT, same texts
 * but for the function name) and copies both lists into device memory.  Blocking; the arrays are not kept. */
int svr_create_draw_list(SvrContext* ctx, const SvrRenderObject* opaque, size_t n_opaque,
                         const SvrRenderObject* transparent, size_t n_transparent, SvrDrawList* out);
/* Replace objects first .. first + n - 1, counted over the opaque list and then the transparent list (an object keeps
 * the list it is in).  Validated like create; first + n beyond the list is SVR_ERR_INVALID_ARGUMENT. */
int svr_update_draw_list(SvrContext* ctx, SvrDrawList list, size_t first, const SvrRenderObject* objs, size_t n);
int svr_destroy_draw_list(SvrContext* ctx, SvrDrawList list);
/* The pass of svr_draw_geometry over the list (see the contract above). */
int svr_draw_list(SvrContext* ctx, SvrDrawList list, const SvrSceneData* scene, SvrStats* out_stats);

/* Test hook: the draw records (DrawDesc, 192 bytes each) and wave chunks (8 bytes each) the last pass ran with, as
 * the device holds them — host-staged or built by a device flatten.  Fences.  *n_draws / *n_chunks receive the
 * counts; draws / chunks may be NULL to query them. */
int svr_debug_read_records(SvrContext* ctx, void* draws, size_t draw_bytes, void* chunks, size_t chunk_bytes,
                           uint32_t* n_draws, uint32_t* n_chunks);

#ifdef __cplusplus
}
#endif
#endif /* SVR_DRAW_LIST_H */
