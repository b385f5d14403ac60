// svr_context.h — what the host files share: the owners of what the runtime hands out, the resources behind the handles,
// the payload of each kind of logged operation, SvrContext itself, and the internal functions that cross files.
//   svr_api.hip     context life cycle, resources, targets, options, read-backs, every geometry entry point
//   svr_log.hip     a pass's submit and retirement, the operation log and its replay
//   svr_screen.hip  the operations over finished targets: depth pyramid, lighting, reflection, post, fog, exposure, temporal, ambient,
//                   overlay, upscaled present
// Host code only.  The C ABI is the extern "C" functions of those files; everything here is internal (namespace svr).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/svr_depth.h"
#include "../../include/svr_draw_list.h"
#include "../../include/svr_attributes.h"
#include "../../include/svr_ids.h"
#include "../../include/svr_lighting.h"
#include "../../include/svr_fog.h"
#include "../../include/svr_dof.h"
#include "../../include/svr_motion.h"
#include "../../include/svr_reflect.h"
#include "../../include/svr_post.h"
#include "../../include/svr_temporal.h"
#include "../../include/svr_ambient.h"
#include "../../include/svr_exposure.h"
#include "../../include/svr_overlay.h"
#include "../../include/svr_load.h"
#include "../../include/svr_occlusion.h"
#include "../../include/svr_views.h"
#include "svr_launch.h"

namespace svr {

int fail(int code, const std::string& msg);  // sets svr_last_error's text (svr_api.hip)
// a failed runtime call: "<what>: <the runtime's text>"
int hip_fail(hipError_t e, const char* what);
// HIPCHK names the failed call by its own text.  HIPCHK_AS: by the text given — where the call goes through one of the
// owners' helpers below, the runtime call it makes, as a caller has always read it in svr_last_error
#define HIPCHK_AS(expr, text)                        \
  do {                                               \
    hipError_t e_ = (expr);                          \
    if (e_ != hipSuccess) return hip_fail(e_, text); \
  } while (0)
#define HIPCHK(expr) HIPCHK_AS(expr, #expr)
// hipMalloc of `bytes` into the DevPtr `owner`
#define DEV_ALLOC(owner, bytes) HIPCHK_AS(dev_alloc(owner, bytes), "hipMalloc((void**)&" #owner ", " #bytes ")")

// Everything the runtime hands out is held by a move-only owner that gives it back: a device allocation, a pinned host
// block, an event, a stream.  Nothing frees by hand; an early return frees what the call had got so far.
struct DevFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
struct PinnedFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
struct EventDestroy {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct StreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
template <class T> using DevPtr = std::unique_ptr<T, DevFree>;
template <class T> using PinnedPtr = std::unique_ptr<T, PinnedFree>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

template <class T> hipError_t dev_alloc(DevPtr<T>& out, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) out.reset(static_cast<T*>(p));
  return e;
}
template <class T> hipError_t pinned_alloc(PinnedPtr<T>& out, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e == hipSuccess) out.reset(static_cast<typename PinnedPtr<T>::pointer>(p));
  return e;
}
inline hipError_t make_event(Event& out, unsigned flags) {
  hipEvent_t ev = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&ev, flags);
  if (e == hipSuccess) out.reset(ev);
  return e;
}

// a device buffer that only grows
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {  // contents are NOT preserved
    if (bytes <= cap) return SVR_OK;
    release();
    size_t want = bytes + bytes / 4;
    HIPCHK(hipMalloc(&p, want));
    cap = want;
    return SVR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct MeshRes {
  DevPtr<SvrVertex> vtx;
  DevPtr<uint32_t> idx;
  DevPtr<float> groups;  // float[6] per 192 indices: box of the vertices they name (setup kernel's chunk culling)
  size_t n_vtx = 0, n_idx = 0;
  bool alive = false;
};
struct ImageRes {
  uint32_t arena_off = 0;   // byte offset of level 0 in the context's texel arena
  size_t bytes = 0;         // all levels
  uint32_t w = 0, h = 0, levels = 0;
  uint32_t lw = 0, lh = 0;  // log2 of the power-of-two padded extent the mip layout is computed from
  uint32_t off[16] = {0};   // = mip_offset(lw, lh, level)
  bool alive = false;
};
struct MaterialRes {
  int pass;
  float cf[4], mr[4];
  uint32_t image, sampler;  // 0-based
};

// One version of a draw list's device copy (include/svr_draw_list.h).  Copy-on-write: svr_update_draw_list makes a
// new one, and the list and every logged pass that was enqueued with this one share it; the last to let go frees it
// (a pass lets go when it is validated, after its completion event — or after its replay).
struct ListVersion {
  DevPtr<SvrRenderObject> dev;  // DRAW ORDER: opaque objects sorted by (material, mesh, submission index), then the transparent ones
  uint32_t n_opaque = 0, n_transparent = 0;
  uint64_t tris_max = 0;  // upper bounds that size the pass's buffers and grids (every object visible)
  size_t chunks_max = 0;
  uint64_t tris_max_opaque = 0;  // ... of the opaque objects alone (depth-only passes: include/svr_depth.h)
  size_t chunks_max_opaque = 0;
  DevPtr<uint32_t> obj_ids;  // [n_opaque] draw order -> position in the opaque array as submitted, + 1 (ID passes: svr_ids.h)
};
struct DrawListRes {
  std::vector<SvrRenderObject> objs;  // submission order: opaque list, then transparent list
  uint32_t n_opaque = 0;
  std::shared_ptr<const ListVersion> cur;
  uint64_t mesh_epoch = 0;  // SvrContext::mesh_epoch when the objects were last validated
  bool valid = false;       // ... and whether they were valid then
  std::string why;          // if not: validate_object's text
  bool alive = false;
};

// A depth pyramid (include/svr_occlusion.h).  The handle, every logged build of it and every logged pass that culls
// against it share its memory; the last to let go frees it (stream-ordered destruction, like a draw list's version).
struct PyramidMem {
  DevPtr<uint32_t> p;  // levels 1 .. levels back to back, level l at word off[l]
  uint32_t levels = 0;
  uint32_t off[PYR_MAX_LEVELS + 1] = {};
  size_t words = 0;
  Event ev_built;  // recorded behind the last build enqueued (the context's stream): stage 1 of a culling pass waits for it
};

// ---------------------------------------------------------------- the entries of the operation log
// One payload type per kind of operation (svr_log.hip "the operation log"): exactly what the kind submits, and submits
// again in a replay.  The entry is a variant of them, so the alternative it holds is the kind and nothing can disagree
// with it.  Only a pass has queues that can overflow, an event and counters of its own.
enum class PassInput { Draws, Objects, List };  // what a pass reads: the one place that says so (P.flatten follows it)
struct PassOp {
  uint32_t seq = 0;  // running number, reported by the device if the pass overflows
  bool timed = false;  // the tile kernel stamps its start and end into the slot's h_clock words: fold into the running mean at retirement
  FrameParams P{};  // parameters as recorded
  PassInput input = PassInput::Draws;
  // what the pass is, as enqueue_pass took it from its PassRequest: the one place submit_pass, retire_pass and the
  // replay read it from.  depth_only: include/svr_depth.h (the setup and tile kernels' depth instances);
  // multiview: include/svr_views.h (P.layer_rows is the kernels' copy of it); depth_load: include/svr_load.h (P.depth_load
  // is the tile launch's copy of it)
  struct Shape {
    bool depth_only = false, multiview = false, depth_load = false;
  } shape;
  std::vector<DrawDesc> draws;  // Draws: records built on the host
  std::vector<SvrRenderObject> objects;  // Objects: the caller's (opaque, then transparent), flattened on the device
  uint32_t n_opaque_obj = 0, n_transparent_obj = 0;  // Objects and List
  // List: the version of a resident draw list it was enqueued with (svr_draw_list): the objects stay on the device
  std::shared_ptr<const ListVersion> list;
  // List, multiview (svr_draw_list_views): the views' viewproj matrices, 16 floats each; empty = one view
  std::vector<float> viewprojs;
  std::shared_ptr<PyramidMem> pyr;  // the pyramid it culls against (include/svr_occlusion.h), or none
  bool flattened() const { return input != PassInput::Draws; }
};
// svr_clear_color, once it runs as a kernel of its own (flush_clear): whole rows of a colour target
struct ClearOp {
  void* target = nullptr;
  int fmt = 0;
  uint32_t row_width = 0, y_first = 0, n_rows = 0;
  uint64_t packed = 0;  // the encoded texel
};
// svr_draw_background: rows [y_first, y_first + n_rows) of a colour target of w x h
struct BackgroundOp {
  void* target = nullptr;
  int fmt = 0;
  uint32_t w = 0, h = 0, y_first = 0, n_rows = 0;
  int effect = 0;
  float data[16] = {};
};
// svr_copy_to_swapchain: the colour target into the swapchain image, destination rows [y_first, row_end)
struct BlitOp {
  const void* src = nullptr;
  int src_fmt = 0;
  uint32_t src_w = 0, src_h = 0;
  void* dst = nullptr;
  uint32_t dst_w = 0, dst_h = 0;
  int dst_fmt = 0;
  uint32_t y_first = 0, n_rows = 0;
  uint32_t rstride = 1, roff = 0, row_end = 0;  // identity blits of an interleaved pass: its tile rows only
  uint32_t* status = nullptr;  // svr_set_present_status: 0 as enqueued, 2 when a replay ran it
};
// svr_build_depth_pyramid: the pyramid it builds, from the depth image src of W x H
struct PyramidOp {
  std::shared_ptr<PyramidMem> pyr;
  const float* src = nullptr;
  uint32_t W = 0, H = 0;
};
// svr_light_pass: the kernel's parameters as recorded, the colour format, its owned tile rows and the caller's lights
struct LightOp {
  LightLaunch launch{};
  int color_fmt = 0;
  uint32_t tiles_y = 0;
  std::vector<SvrPointLight> lights;
};
// svr_post_pass, svr_temporal_resolve (the history roles and validity among them), svr_ambient_pass (the planes it
// reads and writes among them): the kernels' parameters as recorded
using PostOp = PostLaunch;
using TemporalOp = TemporalLaunch;
using AmbientOp = AmbientLaunch;
// svr_meter_exposure: the kernels' parameters as recorded, whether it snaps among them
using ExposureOp = ExposureLaunch;
// svr_draw_overlay: the kernels' parameters as recorded (the device pointers of the copies are filled in at submit) and
// the call's arrays, owned: what a replay uploads again
struct OverlayOp {
  OverlayLaunch launch{};
  uint32_t submitted = 0;  // triangles of every command, for the statistics
  std::vector<SvrOverlayVertex> vertices;
  std::vector<uint16_t> indices;
  std::vector<OverlayCmdDev> cmds;  // those with triangles and a clip box that is not empty
  std::vector<SvrOverlayTexture> textures;
};

// svr_upscale_to_swapchain: the kernel's parameters as recorded, the sharpen's peak by value among them
using UpscaleOp = UpscaleLaunch;
// svr_fog_pass: the kernels' parameters as recorded, by value (the shadow map and the scratch images by address)
struct FogOp {
  FogLaunch launch{};
};
// svr_dof_pass: the kernels' parameters as recorded, by value (the scratch images by address)
struct DofOp {
  DofLaunch launch{};
};
// svr_motion_blur_pass: the kernels' parameters as recorded, by value (the scratch images by address)
struct MotionOp {
  MotionLaunch launch{};
};
// svr_reflect_pass: the kernels' parameters as recorded, by value (the planes and the scratch images by address)
struct ReflectOp {
  ReflectLaunch launch{};
};

struct LoggedOp {
  int slot;  // index into h_counters / op_done / h_stage
  std::variant<PassOp, ClearOp, BackgroundOp, BlitOp, PyramidOp, LightOp, PostOp, TemporalOp, AmbientOp, ExposureOp, OverlayOp, UpscaleOp, FogOp, DofOp, MotionOp, ReflectOp> what;
  template <class Op> LoggedOp(int slot_, Op&& op) : slot(slot_), what(std::forward<Op>(op)) {}
  const PassOp* as_pass() const { return std::get_if<PassOp>(&what); }
};

// The context: SvrContext, the C ABI's opaque type, is this and nothing more (below).
struct Context {
  int device = 0;
  uint32_t W = 0, H = 0;
  int fmt = SVR_COLOR_RGBA16F;
  hipStream_t stream = nullptr;
  DevPtr<void> color_own;
  DevPtr<float> depth_own;
  void* color = nullptr;
  float* depth = nullptr;
  DevPtr<uint2> ids_own;     // svr_enable_ids
  uint2* ids = nullptr;      // the ID target (include/svr_ids.h): a caller's (svr_bind_id_target), ids_own or none
  bool ids_bound = false;    // ... it is the caller's
  DevPtr<void> attr_own[4];  // svr_enable_attributes: the context's planes, by bit number (include/svr_attributes.h)
  void* attr[4] = {};        // the attribute targets: a caller's (svr_bind_attribute_target), attr_own or none
  bool attr_bound[4] = {};   // ... it is the caller's
  uint32_t sx = 0, sy = 0, sw = 0, sh = 0;
  uint32_t rstride = 1, roff = 0;      // svr_set_row_interleave
  int depth_load_op = SVR_DEPTH_CLEAR;  // svr_set_depth_load_op (include/svr_load.h)
  uint32_t* present_status = nullptr;  // svr_set_present_status

  std::vector<MeshRes> meshes;
  std::vector<ImageRes> images;
  std::vector<SvrSamplerDesc> samplers;
  std::vector<MaterialRes> materials;
  std::vector<DrawListRes> lists;  // svr_create_draw_list
  std::vector<std::shared_ptr<PyramidMem>> pyramids;  // svr_create_depth_pyramid (handle - 1; null once destroyed)
  uint32_t occl_bound = 0;                            // svr_set_occlusion_pyramid: the handle passes cull against, 0 = none
  SvrOcclusionStats occl_stats{};                     // of the last instrumented pass
  uint64_t mesh_epoch = 0;         // counts svr_destroy_mesh calls: a draw list re-validates when it has moved
  // Texel arena: every image of the context lives in ONE allocation, so a texel's address is a 32-bit byte
  // offset from one wave-uniform base (FrameParams::tex_arena): the fragment stage's eight gathers per pixel
  // are global loads with an SGPR base and a 32-bit VGPR offset instead of 64-bit pointer arithmetic per tap,
  // and records carry 4 bytes per texture, not a pointer.  Grows by reallocation (device copy, after a
  // fence); offsets never change.  Bound: 4 GiB of texels per context.
  DevPtr<uint8_t> tex_arena;
  size_t tex_arena_cap = 0, tex_arena_top = 0;
  std::vector<std::pair<size_t, size_t>> tex_holes;  // (offset, bytes) of destroyed images, sorted by offset
  DevBuf tex_table;  // TexBinding[materials + 1]; last slot = scratch binding of svr_draw_tex_image
  size_t tex_slots = 0;
  // resource tables of the device flatten pass (k_flatten.hip), rebuilt when a mesh / material was added
  DevBuf mesh_table, mat_table;
  size_t mesh_table_n = 0, mat_table_n = 0;
  int device_flatten = 0;  // SVR_OPT_DEVICE_FLATTEN: 0 auto (>= 2048 objects), 1 always, 2 never

  // Per-pass device buffers, double-buffered: the geometry+binning stage of pass N+1 runs on the
  // internal stream `gstream` while the tile stage of pass N still reads set N on the caller's
  // stream.  ev_bin: set filled (recorded on gstream); ev_tile: set consumed (the pass's op_done event).
  struct PassSet {
    DevBuf inputs, recs, clipq, bigq, tiles, bins, pairs, flat, sorta, occl;  // occl: a culling pass's flag per chunk  // flat: keys / triangle counts / chunk bases of k_flatten  // inputs = DrawDesc[] then WaveChunk[] (one H2D copy)
    Event ev_bin;
    hipEvent_t ev_tile = nullptr;  // not owned: op_done of the pass that used the set last
    bool used = false;
  };
  static const int MAX_OPS = 8;  // operations in flight (log slots)
  static const int NSETS = 4;  // stage 1 of a small pass may run three passes ahead of the tile stage; a large one keeps to one (submit_pass)
  PassSet sets[NSETS];
  int set_pos = 0;
  // the operation log's slots (svr_log.hip): op_done is recorded by passes only
  Event op_done[MAX_OPS];
  int op_pos = 0;
  uint32_t replayed = 0;         // passes re-run by recover_from_overflow
  // svr_clear_color deferred into the next pass (the attachment's loadOp CLEAR): see flush_clear
  struct PendingClear {
    bool valid = false;
    void* target = nullptr;
    uint32_t y0 = 0, rows = 0;
    int fmt = 0;
    uint64_t packed = 0;
  } pending_clear;
  uint32_t next_seq = 1;
  PinnedPtr<uint32_t> h_failed_seq;  // written by the tile kernel of the first failing pass
  DevPtr<uint32_t> d_poison;  // sticky device flag: a pass overflowed, later target writes are void
  Stream gstream;
  Stream gstream_hi;                  // the same at the highest priority: stage 1 of small passes (submit_pass)
  hipStream_t last_g = nullptr;       // the one the previous pass used (not owned)
  Event ev_gswitch;
  DevBuf d_cvt;
  uint32_t clip_cap = 0, extra_cap = 0, bin_cap = 0;
  uint32_t debug_caps = 0;  // SVR_OPT_QUEUE_CAPS
  // pinned host staging + read-back, one of each per operation-log slot
  PinnedPtr<void> h_stage[MAX_OPS];  // per log slot
  size_t h_stage_cap[MAX_OPS] = {};
  PinnedPtr<Counters[]> h_counters;  // [MAX_OPS]
  PinnedPtr<uint32_t> h_row_cost;  // [MAX_OPS][ROW_COST_MAX]: tile-row costs posted by every pass's tile kernel
  PinnedPtr<unsigned long long> h_clock;  // [MAX_OPS][CLOCK_WORDS]: SVR_OPT_KERNEL_TIMING level 1 (FrameParams::host_clock)
  std::vector<uint32_t> row_cost;  // ... of the pass validated last (svr_get_row_costs), with its scissor rows
  uint32_t row_cost_y0 = 0, row_cost_rows = 0;

  // SVR_OPT_KERNEL_TIMING: ring of event quadruples (before setup, after clip, after fill, after tiles)
  static const int TRING = 16;
  Event tev[TRING][5];  // geometry start, after clip, after fill (gstream) | tile start, tile end (stream)
  bool tev_used[TRING] = {};
  bool tev_all[TRING] = {};  // the slot holds all five events (level 2), not just the tile pair
  int tev_pos = 0;
  int kernel_timing = 0;  // 0 off, 1 tile kernel only (it stamps the clock itself: no events), 2 all three stages
  double acc_ms[3] = {0, 0, 0};
  uint32_t acc_n = 0;
  FrameParams last{};        // parameters of the pass enqueued last (debug read-backs)
  uint32_t last_n_draws = 0;  // ... and its draw count, if the host staged its records (svr_debug_read_records)
  bool instrument = false;
  bool tile_cycles = false;
  uint32_t tuning = 0;
  int trace_x = -1, trace_y = -1;
  DevBuf d_trace, d_tile_cycles;
  // svr_light_pass: the device copy of a pass's lights (SVR_MAX_LIGHTS records, refilled in stream order in front of
  // every lighting pass) and the kept-light count per tile of the last one; both allocated once, by the first pass
  DevPtr<SvrPointLight> d_lights;
  DevPtr<uint32_t> d_light_tiles;
  uint32_t light_tiles_n = 0;
  // svr_post_pass: the level images of the bloom (4 halves per texel), sized for the context's extent; allocated once, by
  // the first post pass
  DevPtr<uint2> d_post_levels;
  // svr_fog_pass: the half-resolution images, (S.rgb, T) per block and then t_end per block (fog_blocks of the context's
  // extent each); allocated once, by the first fog pass
  DevPtr<float4> d_fog;
  // svr_dof_pass: the prepared image (dof_texels of the context's extent, 8 bytes each) and then M per cell (dof_cells
  // floats); allocated once, by the first depth of field pass
  DevPtr<uint2> d_dof;
  // svr_motion_blur_pass: the prepared image (motion_texels of the context's extent, 16 bytes each) and then M per cell
  // (motion_cells keys of 8 bytes); allocated once, by the first motion blur pass
  DevPtr<uint4> d_motion;
  // svr_reflect_pass: the trace texels (reflect_texels of the context's extent, 16 bytes each) and then a word per cell
  // (reflect_cells); allocated once, by the first reflection pass
  DevPtr<float4> d_reflect;
  // svr_temporal_resolve: the two history images (4 halves per texel, the context's extent), allocated and zeroed by the
  // first resolve.  temporal_read names the one the next resolve reads; temporal_has: a resolve was accepted, with the
  // scissor temporal_scissor.  All three change at an accepted call only, in call order.
  DevPtr<uint2> d_temporal[2];
  int temporal_read = 0;
  bool temporal_has = false;
  uint32_t temporal_scissor[4] = {0, 0, 0, 0};
  // svr_ambient_pass: the (a, 1/w) scratch plane and the context's own ambient target, both of the context's extent,
  // allocated and zeroed by the first pass that needs them.  ambient_bound: the caller's plane, or null.  light_ao:
  // svr_set_light_ambient_occlusion.
  DevPtr<float2> d_ambient_raw;
  DevPtr<float> d_ambient_own;
  float* ambient_bound = nullptr;
  bool light_ao = false;
  // include/svr_exposure.h: the state, the working bins and the last histogram (EXPOSURE_WORDS words), allocated and
  // initialised by the first call of the group.  exposure_snap: the next accepted meter snaps; it changes at an accepted
  // meter and at svr_reset_exposure only, in call order.  post_auto: svr_set_post_auto_exposure.
  DevPtr<uint32_t> d_exposure;
  bool exposure_snap = true;
  bool post_auto = false;
  // include/svr_overlay.h: the device copy of an overlay's arrays (the statistics at its head) and its triangle records
  // and boxes; allocated by the first overlay, grown when one needs more, refilled in stream order in front of every
  // overlay's kernels
  DevBuf d_overlay_in, d_overlay_recs;
  SvrStats stats{};
  // Declared last, so it goes first: its entries hold draw-list versions and pyramids, and name the memory above.
  std::deque<LoggedOp> log;

  // Every member gives back what it holds, after this: nothing is freed before the device has finished with it.
  ~Context() {
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    if (gstream) (void)hipStreamSynchronize(gstream.get());
    if (gstream_hi) (void)hipStreamSynchronize(gstream_hi.get());
  }
};

}  // namespace svr

struct SvrContext : svr::Context {};

namespace svr {

inline int use_device(SvrContext* ctx) {
  HIPCHK(hipSetDevice(ctx->device));
  return SVR_OK;
}

// the scissor's 32-row tile rows this context renders (svr_set_row_interleave: index % rstride == roff)
inline uint32_t owned_tile_rows(const SvrContext* ctx) {
  const uint32_t all = (ctx->sh + TILE - 1) / TILE;
  return all > ctx->roff ? (all - ctx->roff + ctx->rstride - 1) / ctx->rstride : 0u;
}

// what every present into a swapchain image checks first (svr_copy_to_swapchain, svr_read_swapchain, include/svr_upscale.h)
inline int blit_checks(SvrContext* ctx, const void* dst, uint32_t dw, uint32_t dh, int fmt, const char* who) {
  if (!ctx || !dst) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
  if (dw == 0 || dh == 0 || dw > 16384 || dh > 16384) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(who) + ": extent must be in 1..16384");
  if (fmt != SVR_SWAPCHAIN_B8G8R8A8 && fmt != SVR_SWAPCHAIN_R8G8B8A8) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown format");
  return SVR_OK;
}

// ---------------------------------------------------------------- svr_log.hip
int harvest_timing(SvrContext* ctx, int slot);  // fold one finished slot of the timing ring into the running means
int retire_ops(SvrContext* ctx, bool blocking);
int flush_clear(SvrContext* ctx);     // a deferred svr_clear_color runs now, as a logged operation
int finish_pending(SvrContext* ctx);  // the fence
int poll_pending(SvrContext* ctx);    // validates whatever has finished; never waits
// a free slot of the counters/event/staging ring for the next logged operation (waits if full)
int log_slot(SvrContext* ctx, int* slot);
// log a pass in a free slot, number it and submit it; a pass that could not be submitted is not kept
int log_pass(SvrContext* ctx, PassOp&& pass);
// One submit function for every other kind.  replaying: the operation is run again by recover_from_overflow (a present
// then reports 2 instead of 0)
int submit(SvrContext* ctx, const ClearOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const BackgroundOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const BlitOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const PyramidOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const LightOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const PostOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const TemporalOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const AmbientOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const ExposureOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const OverlayOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const UpscaleOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const FogOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const DofOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const MotionOp& op, int slot, bool replaying);
int submit(SvrContext* ctx, const ReflectOp& op, int slot, bool replaying);
// log the finished payload of any of those kinds in a free slot and submit it; the entry stays in the log if the submit
// fails
template <class Op> int log_op(SvrContext* ctx, Op&& op) {
  static_assert(!std::is_reference_v<Op> && !std::is_same_v<Op, PassOp>, "an rvalue payload; a pass goes through log_pass");
  int slot = 0;
  if (int e = log_slot(ctx, &slot)) return e;
  ctx->log.emplace_back(slot, std::move(op));
  return submit(ctx, std::get<Op>(ctx->log.back().what), slot, false);
}

}  // namespace svr
