// svr_api.hip — the C ABI of include/svr.h over the HIP kernels (host code; no kernels here): the context's life cycle,
// its resources and targets, options and read-backs, and every geometry entry point.
//
// Host half of VulkanEngine::draw_geometry (src/vk_engine.cpp:1357-1477): is_visible cull, sort,
// per-draw records (the push constants + bound buffers of the record lambda, :1412-1457) — or, for
// large object counts, handing the objects to k_flatten.hip — then one pass (svr_log.hip: its kernels, the
// operation log that keeps it until it has fitted its queues).  The operations over finished targets are svr_screen.hip's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <numeric>

#include "svr_context.h"
#include "svr_cull.h"

using namespace svr;

namespace {
thread_local std::string g_err;  // svr_last_error
}
int svr::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int svr::hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? SVR_ERR_OUT_OF_MEMORY : SVR_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

namespace {

// software fp32 -> fp16 (RTE) for the one clear colour the host encodes
uint16_t host_f32_to_f16(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
  if (ax >= 0x7f800000u) return (uint16_t)(sign | (ax > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
  if (ax >= 0x38800000u) {
    uint32_t mant = ax & 0x7fffffu, h = (((ax >> 23) - 112) << 10) | (mant >> 13), rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return (uint16_t)(sign | h);
  }
  if (ax < 0x33000000u) return (uint16_t)sign;
  uint32_t mant = (ax & 0x7fffffu) | 0x800000u;
  int shift = 126 - (int)(ax >> 23);
  uint32_t h = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (h & 1u))) h++;
  return (uint16_t)(sign | h);
}

MeshRes* get_mesh(SvrContext* ctx, SvrMesh h) {
  if (h == 0 || h > ctx->meshes.size() || !ctx->meshes[h - 1].alive) return nullptr;
  return &ctx->meshes[h - 1];
}
ImageRes* get_image(SvrContext* ctx, SvrImage h) {
  if (h == 0 || h > ctx->images.size() || !ctx->images[h - 1].alive) return nullptr;
  return &ctx->images[h - 1];
}

TexBinding make_binding(const ImageRes& im, const SvrSamplerDesc& s) {
  TexBinding tb;
  std::memset(&tb, 0, sizeof(tb));
  uint32_t filters = (uint32_t)s.mag_filter | ((uint32_t)s.min_filter << 1) | ((uint32_t)s.mipmap_mode << 2);
  tb.base_off = im.arena_off;
  tb.pad0 = tex_consts(im.lw, im.lh, im.levels);
  tb.wh = im.w | (im.h << 16);
  tb.info = im.lw | (im.lh << 8) | (im.levels << 16) | (filters << 24);
  // min_lod <= max_lod from here on: the fragment stage's median relies on it.  And -50 <= min_lod, max_lod <= 50 wherever the
  // sampler's range reaches into that interval (binding_lod_range: no result changes): the common-case stage's LOD chain relies
  // on that, and a range that stays outside marks the binding TEX_WIDE_LODS: make_key then withholds the common-case bit.
  if (!binding_lod_range(binding_min_lod(s.min_lod, s.max_lod), s.max_lod, tb.min_lod, tb.max_lod)) tb.info |= TEX_WIDE_LODS << 24;
  return tb;
}

// ---------------------------------------------------------------- texel arena
constexpr size_t ARENA_MAX = (size_t)0xffffff00u;  // offsets are 32-bit
constexpr size_t ARENA_ALIGN = 256;

int arena_alloc(SvrContext* ctx, size_t bytes, uint32_t* off) {
  bytes = (bytes + ARENA_ALIGN - 1) & ~(ARENA_ALIGN - 1);
  for (size_t i = 0; i < ctx->tex_holes.size(); i++) {  // first fit among the holes
    auto& h = ctx->tex_holes[i];
    if (h.second >= bytes) {
      *off = (uint32_t)h.first;
      h.first += bytes;
      h.second -= bytes;
      if (h.second == 0) ctx->tex_holes.erase(ctx->tex_holes.begin() + (long)i);
      return SVR_OK;
    }
  }
  if (ctx->tex_arena_top + bytes > ARENA_MAX)
    return fail(SVR_ERR_OUT_OF_MEMORY, "svr_create_image: more than 4 GiB of texels in one context");
  if (ctx->tex_arena_top + bytes > ctx->tex_arena_cap) {
    // grow: passes in flight read the old arena, so this is a fence; offsets stay valid
    size_t want = std::max(ctx->tex_arena_cap * 2, ctx->tex_arena_top + bytes);
    want = std::min(ARENA_MAX, (want + ((size_t)64 << 20) - 1) & ~(((size_t)64 << 20) - 1));
    if (int e = finish_pending(ctx)) return e;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    DevPtr<uint8_t> grown;
    DEV_ALLOC(grown, want);
    if (ctx->tex_arena_top) {
      hipError_t r = hipMemcpy(grown.get(), ctx->tex_arena.get(), ctx->tex_arena_top, hipMemcpyDeviceToDevice);
      if (r != hipSuccess) return fail(SVR_ERR_DEVICE, std::string("hipMemcpy(texel arena): ") + hipGetErrorString(r));
    }
    ctx->tex_arena = std::move(grown);
    ctx->tex_arena_cap = want;
  }
  *off = (uint32_t)ctx->tex_arena_top;
  ctx->tex_arena_top += bytes;
  return SVR_OK;
}

void arena_free(SvrContext* ctx, size_t off, size_t bytes) {
  bytes = (bytes + ARENA_ALIGN - 1) & ~(ARENA_ALIGN - 1);
  auto& holes = ctx->tex_holes;
  size_t i = 0;
  while (i < holes.size() && holes[i].first < off) i++;
  holes.insert(holes.begin() + (long)i, std::make_pair(off, bytes));
  if (i + 1 < holes.size() && holes[i].first + holes[i].second == holes[i + 1].first) {  // merge with the next
    holes[i].second += holes[i + 1].second;
    holes.erase(holes.begin() + (long)i + 1);
  }
  if (i > 0 && holes[i - 1].first + holes[i - 1].second == holes[i].first) {  // and the previous
    holes[i - 1].second += holes[i].second;
    holes.erase(holes.begin() + (long)i);
  }
  if (!holes.empty() && holes.back().first + holes.back().second == ctx->tex_arena_top) {  // a hole at the top is no hole
    ctx->tex_arena_top = holes.back().first;
    holes.pop_back();
  }
}

// (re)upload the binding table: one slot per material + one scratch slot.  Without a scratch binding only when it is
// stale (a material was added, or svr_draw_tex_image took the scratch slot).
int upload_tex_table(SvrContext* ctx, const TexBinding* scratch) {
  size_t n = ctx->materials.size() + 1;
  if (!scratch && ctx->tex_slots == n) return SVR_OK;
  std::vector<TexBinding> host(n);
  for (size_t i = 0; i < ctx->materials.size(); i++) {
    const MaterialRes& m = ctx->materials[i];
    host[i] = make_binding(ctx->images[m.image], ctx->samplers[m.sampler]);
  }
  if (scratch)
    host[n - 1] = *scratch;
  else
    std::memset(&host[n - 1], 0, sizeof(TexBinding));
  if (ctx->tex_table.cap < n * sizeof(TexBinding)) {
    // the table may be referenced by an in-flight pass: drain before replacing it
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (int e = ctx->tex_table.ensure(n * sizeof(TexBinding) * 2)) return e;
  }
  HIPCHK(hipMemcpyAsync(ctx->tex_table.p, host.data(), n * sizeof(TexBinding), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));  // host vector dies here
  ctx->tex_slots = n;
  return SVR_OK;
}

// ---------------------------------------------------------------- from a drawing call to a pass
// A multiview pass (include/svr_views.h): its layered targets, and the clear its layers start from
struct MultiView {
  uint32_t n_views = 0;
  void* color = nullptr;
  float* depth = nullptr;
  uint2* ids = nullptr;
  bool clear = false;
  uint64_t packed = 0;
};

// What a drawing call asks for.  The entry point makes it (who it is, and whether it draws depth only); check_views
// completes it for a multiview call; whoever learns what the pass draws — run_pass, list_pass, the device flatten of
// draw_geometry — sets the bounds.  From enqueue_pass down it is read only, and nothing takes its parts one by one.
struct PassRequest {
  const char* who = "";                // the entry point: the texts name it
  const SvrSceneData* scene = nullptr;  // the first view's, of a multiview pass; none: svr_draw_colored_triangle / _tex_image
  uint64_t n_tris = 0;                 // bounds on the triangles and wave chunks the pass draws
  size_t n_chunks = 0;
  bool ids = false;         // a geometry pass: it writes the ID and attribute targets that there are
  bool depth_only = false;  // include/svr_depth.h: opaque objects only, no colour
  bool depth_load = false;  // include/svr_load.h: the pass starts from the depth target's contents (take_depth_load_op)
  const MultiView* mv = nullptr;
};
PassRequest geometry_request(const char* who, const SvrSceneData* scene, bool depth_only) {
  PassRequest rq;
  rq.who = who;
  rq.scene = scene;
  rq.ids = true;
  rq.depth_only = depth_only;
  return rq;
}

// What a pass does with a deferred svr_clear_color: Take — it rides along if it covers the pass's rows, else it runs now;
// Flush — it runs now (multiview passes: other targets); Leave — it stays deferred (depth-only passes: the clear belongs
// to the colour target, which they do not touch)
enum class ClearMode { Take, Flush, Leave };
ClearMode clear_mode(const PassRequest& rq) { return rq.depth_only ? ClearMode::Leave : (rq.mv ? ClearMode::Flush : ClearMode::Take); }

// The depth loadOp of a geometry call (include/svr_load.h), decided here and nowhere else, as the context holds it when the
// call is made: single-view colour passes load; multiview and depth-only calls (views: the call is one of the *_views
// entry points) are refused while LOAD is set, before they change anything; svr_draw_colored_triangle and
// svr_draw_tex_image never come here and keep clearing.
int take_depth_load_op(const SvrContext* ctx, PassRequest& rq, bool views) {
  rq.depth_load = false;
  if (ctx->depth_load_op != SVR_DEPTH_LOAD) return SVR_OK;
  if (views || rq.depth_only)
    return fail(SVR_ERR_UNSUPPORTED, std::string(rq.who) + ": " + (views ? "multiview" : "depth-only") + " passes have no SVR_DEPTH_LOAD form (svr_set_depth_load_op)");
  rq.depth_load = true;
  return SVR_OK;
}

// the ID target a pass writes, or none; host records carry object numbers exactly when there is one (a pass under
// SVR_DEPTH_LOAD writes neither IDs nor attribute planes: the G-buffer survives it)
uint2* id_target(const SvrContext* ctx, const PassRequest& rq) { return (!rq.ids || rq.depth_load) ? nullptr : (rq.mv ? rq.mv->ids : ctx->ids); }

// Every parameter of the pass that the request and the context decide, final: the buffers of its set, the log slot and
// the pyramid are submit_pass's.  A multiview pass has every layer's tile rows, layer-major, and its layers' own clear
// rides in it like a deferred one.
int fill_frame_params(SvrContext* ctx, const PassRequest& rq, PassInput input, FrameParams& P) {
  if (rq.n_tris >= 0x3ffffff0ull) return fail(SVR_ERR_UNSUPPORTED, "more than 2^30 triangles in one pass");
  const MultiView* mv = rq.mv;
  std::memset(&P, 0, sizeof(P));
  P.color = rq.depth_only ? nullptr : (mv ? mv->color : ctx->color);
  P.depth = mv ? mv->depth : ctx->depth;
  P.ids = id_target(ctx, rq);
  P.depth_load = rq.depth_load ? 1u : 0u;
  if (rq.ids && !mv && !rq.depth_only && !rq.depth_load)  // attribute planes (include/svr_attributes.h): of single-view shading passes
    for (int i = 0; i < 4; i++) P.attr[i] = ctx->attr[i];
  P.W = ctx->W;
  P.H = ctx->H;
  P.sx = ctx->sx;
  P.sy = ctx->sy;
  P.sw = ctx->sw;
  P.sh = ctx->sh;
  P.tiles_x = (ctx->sw + TILE - 1) / TILE;
  P.rstride = ctx->rstride;
  P.roff = ctx->roff;
  P.layer_rows = mv ? (ctx->H + TILE - 1) / TILE : 0u;
  P.tiles_y = mv ? mv->n_views * P.layer_rows : owned_tile_rows(ctx);
  P.n_tiles = P.tiles_x * P.tiles_y;
  P.n_tris = (uint32_t)rq.n_tris;
  P.n_chunks = (uint32_t)rq.n_chunks;
  P.flatten = input != PassInput::Draws ? 1u : 0u;
  P.tex = (const TexBinding*)ctx->tex_table.p;
  P.tex_arena = ctx->tex_arena.get();
  P.instrument = ctx->instrument ? 1u : 0u;
  P.trace_x = ctx->trace_x;
  P.trace_y = ctx->trace_y;
  // svr_debug_trace_pixel names a pixel of the context's colour target: not one of a layer, and no depth-only pass shades
  P.trace_buf = (ctx->instrument && ctx->trace_x >= 0 && !mv && !rq.depth_only) ? (float*)ctx->d_trace.p : nullptr;
  P.tuning = ctx->tuning;
#ifdef SVR_AB_SPLIT_ALL  // A/B builds only (tools/build_variant.sh): the quarter path for single-view passes of any size
  const bool may_split = !mv || P.n_tiles <= SPLIT_TILES_MAX;
#else
  const bool may_split = P.n_tiles <= SPLIT_TILES_MAX;  // svr_device.h: no tile of a larger pass is worth splitting
#endif
  if (!may_split) P.tuning |= TUNE_NO_SPLIT;
  if (ctx->tile_cycles) {
    if (int e = ctx->d_tile_cycles.ensure((size_t)P.n_tiles * 16)) return e;
    P.tile_cycles = (uint32_t*)ctx->d_tile_cycles.p;
  }
  if (rq.scene) P.scene = *rq.scene;
  if (mv && mv->clear) {
    P.lazy_clear = 1u;
    P.clear_lo = (uint32_t)mv->packed;
    P.clear_hi = (uint32_t)(mv->packed >> 32);
  }
  // a deferred clear of exactly the rows this pass covers rides along; any other one runs now
  const ClearMode clear = clear_mode(rq);
  if (clear == ClearMode::Leave) return SVR_OK;
  const SvrContext::PendingClear& pc = ctx->pending_clear;
  if (clear == ClearMode::Take && pc.valid && pc.target == ctx->color && pc.fmt == ctx->fmt && pc.y0 == ctx->sy && pc.rows == ctx->sh && ctx->sx == 0 &&
      ctx->sw == ctx->W) {
    P.lazy_clear = 1u;
    P.clear_lo = (uint32_t)pc.packed;
    P.clear_hi = (uint32_t)(pc.packed >> 32);
    ctx->pending_clear.valid = false;
  } else if (int e = flush_clear(ctx)) {
    return e;
  }
  return SVR_OK;
}

// (re)upload the handle -> resource tables the device flatten pass reads; its fence leaves a deferred clear deferred
// where the pass does (ClearMode::Leave)
int upload_flatten_tables(SvrContext* ctx, ClearMode clear) {
  if (ctx->mesh_table_n == ctx->meshes.size() && ctx->mat_table_n == ctx->materials.size()) return SVR_OK;
  if (int e = clear == ClearMode::Leave ? retire_ops(ctx, true) : finish_pending(ctx)) return e;  // a pass in flight may be reading the old tables
  std::vector<MeshEntry> me(ctx->meshes.size());
  for (size_t i = 0; i < me.size(); i++) {
    me[i].vtx = ctx->meshes[i].vtx.get();
    me[i].idx = ctx->meshes[i].idx.get();
    me[i].groups = ctx->meshes[i].groups.get();
    me[i].pad = 0;
  }
  std::vector<MatEntry> ma(ctx->materials.size());
  for (size_t i = 0; i < ma.size(); i++) {
    std::memset(&ma[i], 0, sizeof(MatEntry));
    std::memcpy(ma[i].cf, ctx->materials[i].cf, 16);
    ma[i].pass = (uint32_t)ctx->materials[i].pass;
  }
  if (int e = ctx->mesh_table.ensure(std::max<size_t>(me.size() * sizeof(MeshEntry), 256))) return e;
  if (int e = ctx->mat_table.ensure(std::max<size_t>(ma.size() * sizeof(MatEntry), 256))) return e;
  if (!me.empty()) HIPCHK(hipMemcpy(ctx->mesh_table.p, me.data(), me.size() * sizeof(MeshEntry), hipMemcpyHostToDevice));
  if (!ma.empty()) HIPCHK(hipMemcpy(ctx->mat_table.p, ma.data(), ma.size() * sizeof(MatEntry), hipMemcpyHostToDevice));
  ctx->mesh_table_n = me.size();
  ctx->mat_table_n = ma.size();
  return SVR_OK;
}

// Enqueue the pass rq asks for.  `in` holds its input (in.input and the draws, objects or list version it names).
int enqueue_pass(SvrContext* ctx, const PassRequest& rq, PassOp&& in) {
  if (int e = poll_pending(ctx)) return e;
  if (in.flattened())  // before fill_frame_params: it can fence, and so flush the deferred clear
    if (int e = upload_flatten_tables(ctx, clear_mode(rq))) return e;
  const SvrContext::PendingClear asked = ctx->pending_clear;  // folded into P.lazy_clear below: put back if the pass is not enqueued
  if (int e = fill_frame_params(ctx, rq, in.input, in.P)) return e;
  const bool took_clear = in.P.lazy_clear && !rq.mv;
  in.shape.depth_only = rq.depth_only;
  in.shape.multiview = rq.mv != nullptr;
  in.shape.depth_load = rq.depth_load;
  if (ctx->occl_bound && !rq.mv) in.pyr = ctx->pyramids[ctx->occl_bound - 1];  // (multiview passes refuse a bound pyramid)
  const int e = log_pass(ctx, std::move(in));
  if (e && took_clear) ctx->pending_clear = asked;
  return e;
}

// a pass of draw records built on the host: numbers their triangles and swaps them into the log
int run_pass(SvrContext* ctx, PassRequest& rq, std::vector<DrawDesc>& draws) {
  rq.n_tris = 0;
  rq.n_chunks = 0;
  for (DrawDesc& d : draws) {
    d.tri_base = (uint32_t)rq.n_tris;
    rq.n_tris += d.tri_count;
    rq.n_chunks += chunk_count(d.first_index, d.tri_count);
  }
  PassOp in;
  in.draws.swap(draws);
  return enqueue_pass(ctx, rq, std::move(in));
}

// the device flatten's bound on the objects of one pass, and so on those of a draw list (include/svr_draw_list.h)
constexpr size_t FLATTEN_MAX_OBJECTS = 16384;

// upper bounds on the triangles and wave chunks of a flattened pass over these objects (every object visible): they size
// the pass's buffers and grids
void add_object_bounds(const SvrRenderObject* objs, size_t n, uint64_t* tris, size_t* chunks) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = objs[i].index_count / 3u;
    *tris += t;
    *chunks += chunk_count(objs[i].first_index, t);
  }
}

// draw order of opaque objects (src/vk_engine.cpp:1369-1378): indices into objs, sorted by the deterministic key
// (material, mesh, submission index).  The index is part of the key, so the order is a stable sort's without its buffer
void sort_draw_order(std::vector<uint32_t>& order, const SvrRenderObject* objs) {
  std::sort(order.begin(), order.end(), [objs](uint32_t ia, uint32_t ib) {
    const SvrRenderObject& a = objs[ia];
    const SvrRenderObject& b = objs[ib];
    if (a.material != b.material) return a.material < b.material;
    if (a.mesh != b.mesh) return a.mesh < b.mesh;
    return ia < ib;
  });
}

// the end of a drawing call: its stats become the context's and the caller's; t0: when the call began (mesh_draw_time)
int finish_draw(SvrContext* ctx, SvrStats st, SvrStats* out_stats, int e,
                const std::chrono::steady_clock::time_point* t0 = nullptr) {
  if (t0) st.mesh_draw_time = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - *t0).count();
  ctx->stats = st;
  if (out_stats) *out_stats = st;
  return e;
}

// interleaved rows and more ranks than tile rows: this context owns no tile row, and a geometry pass draws nothing
// (a depth-only pass leaves a deferred clear of the colour target as it is)
bool owns_nothing(SvrContext* ctx, SvrStats* out_stats, const PassRequest& rq) {
  if (owned_tile_rows(ctx) != 0) return false;
  if (clear_mode(rq) != ClearMode::Leave) ctx->pending_clear.valid = false;
  finish_draw(ctx, SvrStats{}, out_stats, SVR_OK);
  return true;
}

}  // namespace

// ================================================================================================
extern "C" {

const char* svr_last_error(void) { return g_err.c_str(); }
const char* svr_backend_name(void) { return "hip-gfx950"; }

int svr_create(const SvrConfig* cfg, SvrContext** out) {
  if (!cfg || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create: null argument");
  if (cfg->width == 0 || cfg->height == 0 || cfg->width > 16384 || cfg->height > 16384)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create: extent must be in 1..16384");
  if (cfg->color_format != SVR_COLOR_RGBA16F && cfg->color_format != SVR_COLOR_RGBA8)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create: unknown colour format");
  int n_dev = 0;
  hipError_t e = hipGetDeviceCount(&n_dev);
  if (e != hipSuccess || n_dev <= 0)
    return fail(SVR_ERR_DEVICE, std::string("svr_create: no HIP device (") + hipGetErrorString(e) +
                                    "); this library has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= n_dev) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create: bad device ordinal");
  HIPCHK(hipSetDevice(cfg->device));
  std::unique_ptr<SvrContext> ctx(new SvrContext());  // a failure below gives back what the context has got so far
  ctx->device = cfg->device;
  ctx->W = cfg->width;
  ctx->H = cfg->height;
  ctx->fmt = cfg->color_format;
  ctx->sw = ctx->W;
  ctx->sh = ctx->H;
  size_t n = (size_t)ctx->W * ctx->H;
  size_t cbytes = n * (ctx->fmt == SVR_COLOR_RGBA16F ? 8 : 4);
  HIPCHK_AS(dev_alloc(ctx->color_own, cbytes), "hipMalloc(color)");
  HIPCHK_AS(dev_alloc(ctx->depth_own, n * 4), "hipMalloc(depth)");
  HIPCHK_AS(hipMemset(ctx->color_own.get(), 0, cbytes), "hipMemset(color)");
  HIPCHK_AS(hipMemset(ctx->depth_own.get(), 0, n * 4), "hipMemset(depth)");
  ctx->color = ctx->color_own.get();
  ctx->depth = ctx->depth_own.get();
  // (the internal streams are made by the first pass that needs them: submit_pass)
  HIPCHK_AS(make_event(ctx->ev_gswitch, hipEventDisableTiming), "hipEventCreate");
  for (SvrContext::PassSet& set : ctx->sets)
    HIPCHK_AS(make_event(set.ev_bin, hipEventDisableTiming), "hipEventCreate");
  HIPCHK_AS(pinned_alloc(ctx->h_counters, sizeof(Counters) * SvrContext::MAX_OPS), "hipHostMalloc");
  for (Event& ev : ctx->op_done)
    HIPCHK_AS(make_event(ev, hipEventDefault), "hipEventCreate");
  HIPCHK_AS(pinned_alloc(ctx->h_row_cost, sizeof(uint32_t) * ROW_COST_MAX * SvrContext::MAX_OPS), "hipHostMalloc");
  std::memset(ctx->h_row_cost.get(), 0, sizeof(uint32_t) * ROW_COST_MAX * SvrContext::MAX_OPS);
  HIPCHK_AS(pinned_alloc(ctx->h_clock, sizeof(unsigned long long) * CLOCK_WORDS * SvrContext::MAX_OPS), "hipHostMalloc");
  std::memset(ctx->h_clock.get(), 0, sizeof(unsigned long long) * CLOCK_WORDS * SvrContext::MAX_OPS);
  HIPCHK_AS(pinned_alloc(ctx->h_failed_seq, 64), "hipHostMalloc");
  *ctx->h_failed_seq = 0;
  HIPCHK_AS(dev_alloc(ctx->d_poison, 256), "hipMalloc");
  HIPCHK_AS(hipMemset(ctx->d_poison.get(), 0, 256), "hipMemset");
  *out = ctx.release();
  return SVR_OK;
}

void svr_destroy(SvrContext* ctx) { delete ctx; }  // ~SvrContext: the fence, then every member lets go

int svr_set_stream(SvrContext* ctx, void* hip_stream) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;  // work on the old stream must not be orphaned
  ctx->stream = (hipStream_t)hip_stream;
  return SVR_OK;
}

int svr_bind_targets(SvrContext* ctx, void* color_dev, void* depth_dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if ((color_dev == nullptr) != (depth_dev == nullptr))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_bind_targets: pass both targets or both NULL");
  if (int e = use_device(ctx)) return e;
  // no fence: passes already enqueued carry their own target pointers (also for a replay), so frames
  // can alternate between target sets while earlier ones are still in flight
  if (int e = poll_pending(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;  // a deferred clear belongs to the targets it was asked for
  ctx->color = color_dev ? color_dev : ctx->color_own.get();
  ctx->depth = depth_dev ? (float*)depth_dev : ctx->depth_own.get();
  return SVR_OK;
}

int svr_get_targets(SvrContext* ctx, void** color_dev, void** depth_dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (int e = use_device(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;  // the caller is about to look at the memory itself
  if (color_dev) *color_dev = ctx->color;
  if (depth_dev) *depth_dev = ctx->depth;
  return SVR_OK;
}

int svr_upload_mesh(SvrContext* ctx, const uint32_t* indices, size_t n_indices, const SvrVertex* vertices,
                    size_t n_vertices, SvrMesh* out) {
  if (!ctx || !out || (!indices && n_indices) || (!vertices && n_vertices))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_upload_mesh: null argument");
  if (n_vertices > 0xffffffffull || n_indices > 0xffffffffull)
    return fail(SVR_ERR_UNSUPPORTED, "svr_upload_mesh: more than 2^32 elements");
  for (size_t i = 0; i < n_indices; i++)
    if (indices[i] >= n_vertices) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_upload_mesh: index out of range");
  if (int e = use_device(ctx)) return e;
  MeshRes m;
  // device-local vertex + index buffers, blocking staged copy (src/vk_engine.cpp:345-381)
  DEV_ALLOC(m.vtx, std::max<size_t>(n_vertices * sizeof(SvrVertex), 64));
  hipError_t r = dev_alloc(m.idx, std::max<size_t>(n_indices * 4, 64));
  if (r != hipSuccess) return fail(SVR_ERR_OUT_OF_MEMORY, std::string("hipMalloc(indices): ") + hipGetErrorString(r));
  if (n_vertices) HIPCHK(hipMemcpy(m.vtx.get(), vertices, n_vertices * sizeof(SvrVertex), hipMemcpyHostToDevice));
  if (n_indices) HIPCHK(hipMemcpy(m.idx.get(), indices, n_indices * 4, hipMemcpyHostToDevice));
  // Index-group boxes: min / max position of the vertices named by every 192 consecutive indices.  A wave of the
  // setup kernel handles 64 consecutive triangles of a draw, i.e. at most two such groups, and skips them when
  // their box cannot reach the scissor.  (The bounds a caller attaches to a RenderObject are the loader's —
  // src/vk_loader.cpp:366-375, over all vertices of the mesh so far — and only is_visible may trust them.)
  {
    const size_t n_groups = (n_indices + GROUP_INDICES - 1) / GROUP_INDICES;
    std::vector<float> boxes(std::max<size_t>(n_groups, 1) * GROUP_WORDS);
    for (size_t g = 0; g < n_groups; g++) {
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      uint32_t vmin = 0xffffffffu, vmax = 0u;  // the vertices the group names: the setup kernel stages that range through LDS
      const size_t end = std::min(n_indices, (g + 1) * GROUP_INDICES);
      for (size_t i = g * GROUP_INDICES; i < end; i++) {
        vmin = std::min(vmin, indices[i]);
        vmax = std::max(vmax, indices[i]);
        const float* p = vertices[indices[i]].position;
        for (int k = 0; k < 3; k++) {
          lo[k] = p[k] < lo[k] ? p[k] : lo[k];
          hi[k] = p[k] > hi[k] ? p[k] : hi[k];
          if (!std::isfinite(p[k])) lo[k] = hi[k] = NAN;  // poisons the box for good (comparisons with NaN are false): the kernel never culls on it
        }
      }
      for (int k = 0; k < 3; k++) {
        boxes[g * GROUP_WORDS + k] = lo[k];
        boxes[g * GROUP_WORDS + 3 + k] = hi[k];
      }
      std::memcpy(&boxes[g * GROUP_WORDS + 6], &vmin, 4);
      std::memcpy(&boxes[g * GROUP_WORDS + 7], &vmax, 4);
    }
    hipError_t rg = dev_alloc(m.groups, boxes.size() * sizeof(float));
    if (rg == hipSuccess) rg = hipMemcpy(m.groups.get(), boxes.data(), boxes.size() * sizeof(float), hipMemcpyHostToDevice);
    if (rg != hipSuccess) return fail(SVR_ERR_OUT_OF_MEMORY, std::string("svr_upload_mesh: index-group boxes: ") + hipGetErrorString(rg));
  }
  m.n_vtx = n_vertices;
  m.n_idx = n_indices;
  m.alive = true;
  ctx->meshes.push_back(std::move(m));
  *out = (SvrMesh)ctx->meshes.size();
  return SVR_OK;
}

int svr_destroy_mesh(SvrContext* ctx, SvrMesh mesh) {
  MeshRes* m = ctx ? get_mesh(ctx, mesh) : nullptr;
  if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_destroy_mesh: bad handle");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  m->vtx.reset();
  m->idx.reset();
  m->groups.reset();
  m->alive = false;
  ctx->mesh_epoch++;  // draw lists that name it fail at their next svr_draw_list
  return SVR_OK;
}

int svr_create_image(SvrContext* ctx, const void* rgba8, uint32_t width, uint32_t height, int mipmapped,
                     SvrImage* out) {
  if (!ctx || !rgba8 || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_image: null argument");
  if (width == 0 || height == 0 || width > 16384 || height > 16384)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_image: extent must be in 1..16384");
  if (int e = use_device(ctx)) return e;
  ImageRes im;
  im.w = width;
  im.h = height;
  im.levels = 1;
  if (mipmapped) {  // src/vk_engine.cpp:1543-1545
    uint32_t m = std::max(width, height);
    while (m > 1) {
      m >>= 1;
      im.levels++;
    }
  }
  // Mip levels are laid out as if the image were padded to 2^lw x 2^lh and every level to whole tiles, so a shader
  // derives a level's offset from (lw, lh, level) alone (svr::mip_offset) and needs no per-image table.
  while ((1u << im.lw) < width) im.lw++;
  while ((1u << im.lh) < height) im.lh++;
  for (uint32_t l = 0; l < im.levels; l++) im.off[l] = mip_offset(im.lw, im.lh, l);
  uint32_t lw = width, lh = height;
  if (im.lw + im.lh > 28) return fail(SVR_ERR_UNSUPPORTED, "svr_create_image: image larger than 1 GiB");
  const size_t total = (size_t)mip_offset(im.lw, im.lh, im.levels - 1) + level_bytes(im.lw, im.lh, im.levels - 1);
  im.bytes = std::max<size_t>(total, 256);
  // the linear host image goes through a staging buffer; one kernel scatters it into level 0's tiles
  const size_t linear = (size_t)width * height * 4;
  DevPtr<uint8_t> staging;
  if (dev_alloc(staging, linear) != hipSuccess) return fail(SVR_ERR_OUT_OF_MEMORY, "svr_create_image: staging buffer");
  if (int e = arena_alloc(ctx, im.bytes, &im.arena_off)) return e;
  uint8_t* base = ctx->tex_arena.get() + im.arena_off;
  hipError_t r = hipMemcpy(staging.get(), rgba8, linear, hipMemcpyHostToDevice);
  if (r != hipSuccess) {
    arena_free(ctx, im.arena_off, im.bytes);
    return fail(SVR_ERR_DEVICE, std::string("hipMemcpy(image): ") + hipGetErrorString(r));
  }
  launch_retile(true, staging.get(), base, width, height, level_lw(im.lw, 0), ctx->stream);
  // generate_mipmaps: level n -> n+1, each a 2:1 linear blit (src/vk_images.cpp:66-133)
  lw = width;
  lh = height;
  for (uint32_t l = 1; l < im.levels; l++) {
    uint32_t dw = std::max(1u, lw >> 1), dh = std::max(1u, lh >> 1);
    launch_downsample(base + im.off[l - 1], lw, lh, level_lw(im.lw, l - 1), base + im.off[l], dw, dh, level_lw(im.lw, l), ctx->stream);
    lw = dw;
    lh = dh;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));  // immediate_submit is blocking (src/vk_engine.cpp:1110-1129)
  im.alive = true;
  ctx->images.push_back(im);
  *out = (SvrImage)ctx->images.size();
  return SVR_OK;
}

int svr_destroy_image(SvrContext* ctx, SvrImage image) {
  ImageRes* im = ctx ? get_image(ctx, image) : nullptr;
  if (!im) return fail(SVR_ERR_BAD_HANDLE, "svr_destroy_image: bad handle");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  arena_free(ctx, im->arena_off, im->bytes);
  im->alive = false;
  return SVR_OK;
}

int svr_read_image_level(SvrContext* ctx, SvrImage image, uint32_t level, void* dst, size_t bytes, uint32_t* w,
                         uint32_t* h) {
  ImageRes* im = ctx ? get_image(ctx, image) : nullptr;
  if (!im) return fail(SVR_ERR_BAD_HANDLE, "svr_read_image_level: bad handle");
  if (level >= im->levels) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_image_level: no such level");
  uint32_t lw = std::max(1u, im->w >> level), lh = std::max(1u, im->h >> level);
  if (w) *w = lw;
  if (h) *h = lh;
  if (dst) {
    size_t need = (size_t)lw * lh * 4;
    if (bytes < need) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_image_level: buffer too small");
    if (int e = use_device(ctx)) return e;
    DevPtr<uint8_t> staging;  // the level's tiles gathered back into linear rows
    if (dev_alloc(staging, need) != hipSuccess) return fail(SVR_ERR_OUT_OF_MEMORY, "svr_read_image_level: staging buffer");
    launch_retile(false, staging.get(), ctx->tex_arena.get() + im->arena_off + im->off[level], lw, lh, level_lw(im->lw, level), ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(dst, staging.get(), need, hipMemcpyDeviceToHost));
  }
  return SVR_OK;
}

int svr_create_sampler(SvrContext* ctx, const SvrSamplerDesc* desc, SvrSampler* out) {
  if (!ctx || !desc || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_sampler: null argument");
  if ((desc->mag_filter | 1) != 1 || (desc->min_filter | 1) != 1 || (desc->mipmap_mode | 1) != 1)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_sampler: bad filter enum");
  if (!(desc->min_lod <= desc->max_lod)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_sampler: min_lod > max_lod");
  ctx->samplers.push_back(*desc);
  *out = (SvrSampler)ctx->samplers.size();
  return SVR_OK;
}

int svr_write_material(SvrContext* ctx, int pass, const float color_factors[4], const float metal_rough_factors[4],
                       SvrImage color_image, SvrSampler color_sampler, SvrMaterial* out) {
  if (!ctx || !color_factors || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_write_material: null argument");
  if (!get_image(ctx, color_image)) return fail(SVR_ERR_BAD_HANDLE, "svr_write_material: bad image");
  if (color_sampler == 0 || color_sampler > ctx->samplers.size())
    return fail(SVR_ERR_BAD_HANDLE, "svr_write_material: bad sampler");
  if (pass < 0 || pass > 2) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_write_material: bad pass");
  if (int e = use_device(ctx)) return e;
  MaterialRes m;
  m.pass = pass;
  for (int i = 0; i < 4; i++) {
    m.cf[i] = color_factors[i];
    m.mr[i] = metal_rough_factors ? metal_rough_factors[i] : 0.0f;
  }
  m.image = color_image - 1;
  m.sampler = color_sampler - 1;
  ctx->materials.push_back(m);
  ctx->tex_slots = 0;  // table is stale; rebuilt lazily at the next draw
  *out = (SvrMaterial)ctx->materials.size();
  return SVR_OK;
}

// the texel a clear colour is stored as in the context's colour format
static uint64_t encode_clear(const SvrContext* ctx, const float rgba[4]) {
  uint64_t packed;
  if (ctx->fmt == SVR_COLOR_RGBA16F) {
    packed = (uint64_t)host_f32_to_f16(rgba[0]) | ((uint64_t)host_f32_to_f16(rgba[1]) << 16) |
             ((uint64_t)host_f32_to_f16(rgba[2]) << 32) | ((uint64_t)host_f32_to_f16(rgba[3]) << 48);
  } else {
    packed = 0;
    for (int k = 0; k < 4; k++) {
      float c = rgba[k];
      if (!(c == c)) c = 0.0f;
      c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
      packed |= (uint64_t)(uint32_t)std::nearbyintf(c * 255.0f) << (8 * k);
    }
  }
  return packed;
}

int svr_clear_color(SvrContext* ctx, const float rgba[4]) {
  if (!ctx || !rgba) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_clear_color: null argument");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  const uint64_t packed = encode_clear(ctx, rgba);
  // whole rows of the scissor (a rank of the multi-GPU path only owns its band); deferred (flush_clear)
  if (int e = flush_clear(ctx)) return e;  // an older deferred clear cannot be skipped in general
  ctx->pending_clear.valid = true;
  ctx->pending_clear.target = ctx->color;
  ctx->pending_clear.y0 = ctx->sy;
  ctx->pending_clear.rows = ctx->sh;
  ctx->pending_clear.fmt = ctx->fmt;
  ctx->pending_clear.packed = packed;
  if (ctx->tuning & TUNE_NO_LAZY_CLEAR) return flush_clear(ctx);
  return SVR_OK;
}

int svr_draw_background(SvrContext* ctx, int effect, const float data[16]) {
  if (!ctx || !data) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_background: null argument");
  if (effect != SVR_BACKGROUND_GRADIENT && effect != SVR_BACKGROUND_SKY)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_background: unknown effect");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;
  BackgroundOp op;
  op.target = ctx->color;
  op.fmt = ctx->fmt;
  op.w = ctx->W;
  op.h = ctx->H;
  op.y_first = ctx->sy;
  op.n_rows = ctx->sh;
  op.effect = effect;
  std::memcpy(op.data, data, sizeof(op.data));
  return log_op(ctx, std::move(op));
}

int svr_copy_to_swapchain(SvrContext* ctx, void* dst_dev, uint32_t dw, uint32_t dh, int fmt) {
  if (int e = blit_checks(ctx, dst_dev, dw, dh, fmt, "svr_copy_to_swapchain")) return e;
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;
  // identity extent: the rows of the scissor (a rank of the multi-GPU path presents its band); scaled: everything
  const bool identity = dw == ctx->W && dh == ctx->H;
  BlitOp op;
  op.src = ctx->color;
  op.src_fmt = ctx->fmt;
  op.src_w = ctx->W;
  op.src_h = ctx->H;
  op.dst = dst_dev;
  op.dst_w = dw;
  op.dst_h = dh;
  op.dst_fmt = fmt;
  op.y_first = identity ? ctx->sy : 0u;
  op.n_rows = identity ? ctx->sh : dh;
  op.row_end = op.y_first + op.n_rows;
  if (identity && ctx->rstride > 1u) {  // a rank of the interleaved form presents its own tile rows, in place
    op.rstride = ctx->rstride;
    op.roff = ctx->roff;
    op.n_rows = owned_tile_rows(ctx) * TILE;
  }
  op.status = ctx->present_status;
  return log_op(ctx, std::move(op));
}

int svr_read_swapchain(SvrContext* ctx, uint32_t dw, uint32_t dh, int fmt, void* dst_host, size_t bytes) {
  if (int e = blit_checks(ctx, dst_host, dw, dh, fmt, "svr_read_swapchain")) return e;
  if (bytes < (size_t)dw * dh * 4) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_swapchain: buffer too small");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;  // the read-back is a fence
  if (int e = ctx->d_cvt.ensure((size_t)dw * dh * 4)) return e;
  launch_blit(ctx->color, ctx->fmt, ctx->W, ctx->H, ctx->d_cvt.p, dw, dh, 0, dh, fmt, ctx->d_poison.get(), 1u, 0u, dh, nullptr, 0u, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst_host, ctx->d_cvt.p, (size_t)dw * dh * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_set_scissor(SvrContext* ctx, uint32_t x, uint32_t y, uint32_t w, uint32_t h) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (w == 0 || h == 0 || (uint64_t)x + w > ctx->W || (uint64_t)y + h > ctx->H)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_scissor: rectangle outside the target");
  ctx->sx = x;
  ctx->sy = y;
  ctx->sw = w;
  ctx->sh = h;
  return SVR_OK;
}

// include/svr_load.h
int svr_set_depth_load_op(SvrContext* ctx, int op) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (op != SVR_DEPTH_CLEAR && op != SVR_DEPTH_LOAD) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_depth_load_op: op must be SVR_DEPTH_CLEAR or SVR_DEPTH_LOAD");
  ctx->depth_load_op = op;
  return SVR_OK;
}

int svr_get_depth_load_op(SvrContext* ctx, int* op) {
  if (!ctx || !op) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_depth_load_op: null argument");
  *op = ctx->depth_load_op;
  return SVR_OK;
}

int svr_set_row_interleave(SvrContext* ctx, uint32_t stride, uint32_t offset) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (stride == 0 || stride > 64 || offset >= stride) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_row_interleave: need 1 <= stride <= 64, offset < stride");
  ctx->rstride = stride;
  ctx->roff = offset;
  return SVR_OK;
}

int svr_set_present_status(SvrContext* ctx, uint32_t* status_dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  ctx->present_status = status_dev;
  return SVR_OK;
}

// who: the entry point the texts name (svr_draw_geometry, or the draw-list calls that apply the same rules)
static int validate_object(SvrContext* ctx, const SvrRenderObject& o, bool transparent_list, const char* who = "svr_draw_geometry") {
  const char* which = transparent_list ? "transparent" : "opaque";
  const std::string fn(who);
  MeshRes* m = get_mesh(ctx, o.mesh);
  if (!m) return fail(SVR_ERR_BAD_HANDLE, fn + ": bad mesh handle in " + which);
  if (o.material == 0 || o.material > ctx->materials.size())
    return fail(SVR_ERR_BAD_HANDLE, fn + ": bad material handle in " + which);
  if ((uint64_t)o.first_index + o.index_count > m->n_idx)
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": index range outside the mesh in " + which);
  // MeshNode::Draw routes by pass_type (src/vk_engine.cpp:1729-1733)
  bool is_tr = ctx->materials[o.material - 1].pass == SVR_PASS_TRANSPARENT;
  if (is_tr && !transparent_list)
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": Transparent material in the opaque list");
  if (!is_tr && transparent_list)
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": non-Transparent material in the transparent list");
  return SVR_OK;
}

// DrawDesc::mvp = viewproj * mat, column by column as prologue_kernel's matvec4 forms it (C0): the product then is the
// one a single-view pass over this scene computes on the device
static void host_mvp(const float* vp, const float* mat, float* out) {
  for (int j = 0; j < 4; j++)
    for (int r = 0; r < 4; r++) {
      float acc = vp[0 + r] * mat[4 * j + 0];
      acc = std::fmaf(vp[4 + r], mat[4 * j + 1], acc);
      acc = std::fmaf(vp[8 + r], mat[4 * j + 2], acc);
      acc = std::fmaf(vp[12 + r], mat[4 * j + 3], acc);
      out[4 * j + r] = acc;
    }
}

// what every record that draws from a mesh holds: its matrix, buffers and index range, a slot of the binding table, flags
static DrawDesc mesh_record(const MeshRes& m, const float mat[16], uint32_t first_index, uint32_t index_count, uint32_t tex, uint32_t flags) {
  DrawDesc d;
  std::memset(&d, 0, sizeof(d));
  std::memcpy(d.mat, mat, 64);
  d.vtx = m.vtx.get();
  d.idx = m.idx.get() + first_index;
  d.groups = m.groups.get();
  d.first_index = first_index;
  d.tri_count = index_count / 3;
  d.tex = tex;
  d.flags = flags;
  return d;
}

// The record of one mesh object (the push constants + bound buffers of the record lambda, src/vk_engine.cpp:1412-1457).
// object: its number for the ID target (include/svr_ids.h), 0 = none.  viewproj: the view's, of a multiview pass, whose
// mvp the host computes; null: a single-view pass leaves DrawDesc::mvp to the prologue kernel (n_draws of launch_prologue)
static DrawDesc object_record(const SvrContext* ctx, const SvrRenderObject& o, uint32_t object, uint32_t view, const float* viewproj) {
  const MaterialRes& mat = ctx->materials[o.material - 1];
  DrawDesc d = mesh_record(ctx->meshes[o.mesh - 1], o.transform, o.first_index, o.index_count, o.material - 1,
                           ((uint32_t)PIPE_MESH << F_KIND_SHIFT) | (mat.pass == SVR_PASS_TRANSPARENT ? F_TRANSPARENT : 0u) | (view << F_VIEW_SHIFT));
  if (viewproj) host_mvp(viewproj, d.mat, d.mvp);
  std::memcpy(d.color_factors, mat.cf, 16);
  d.pad = object;
  return d;
}

// The host path of every geometry call, for the one view of rq.scene or the views of a multiview request (scenes[k]):
// each view culls its opaque objects (src/vk_engine.cpp:1361-1367) and sorts the visible ones into draw order, then gets
// its draws, opaque before transparent, view after view; triangle numbers and wave chunks run on across the views (run_pass)
static int draw_objects(SvrContext* ctx, PassRequest& rq, const SvrSceneData* scenes, const SvrRenderObject* opaque, size_t n_opaque,
                        const SvrRenderObject* transparent, size_t n_transparent, SvrStats* out_stats,
                        const std::chrono::steady_clock::time_point& t0) {
  const uint32_t n_views = rq.mv ? rq.mv->n_views : 1u;
  const bool ids = id_target(ctx, rq) != nullptr;  // DrawDesc::pad = the opaque object's number
  std::vector<uint32_t> order;
  order.reserve(n_opaque);
  std::vector<DrawDesc> draws;
  SvrStats st{};
  for (uint32_t k = 0; k < n_views; k++) {
    const float* vp = scenes[k].viewproj;
    order.clear();
    for (size_t i = 0; i < n_opaque; i++)
      if (is_visible(opaque[i], vp)) order.push_back((uint32_t)i);
    sort_draw_order(order, opaque);
    if (k == 0) draws.reserve((order.size() + n_transparent) * n_views);
    auto push = [&](const SvrRenderObject& o, uint32_t object) {
      draws.push_back(object_record(ctx, o, object, k, rq.mv ? vp : nullptr));
      st.drawcall_count++;
      st.triangle_count += (int)(o.index_count / 3);
    };
    for (uint32_t i : order) push(opaque[i], ids ? i + 1u : 0u);
    for (size_t i = 0; i < n_transparent; i++) push(transparent[i], 0u);
    st.culled_draws += (uint32_t)(n_opaque - order.size());
  }
  return finish_draw(ctx, st, out_stats, run_pass(ctx, rq, draws), &t0);
}

// svr_draw_geometry and svr_draw_depth (no transparent objects then)
static int draw_geometry(SvrContext* ctx, PassRequest rq, const SvrRenderObject* opaque, size_t n_opaque, const SvrRenderObject* transparent,
                         size_t n_transparent, SvrStats* out_stats) {
  if (!ctx || !rq.scene || (!opaque && n_opaque) || (!transparent && n_transparent))
    return fail(SVR_ERR_INVALID_ARGUMENT, std::string(rq.who) + ": null argument");
  if (int e = take_depth_load_op(ctx, rq, false)) return e;
  auto t0 = std::chrono::steady_clock::now();
  if (int e = use_device(ctx)) return e;
  for (size_t i = 0; i < n_opaque; i++)
    if (int e = validate_object(ctx, opaque[i], false, rq.who)) return e;
  for (size_t i = 0; i < n_transparent; i++)
    if (int e = validate_object(ctx, transparent[i], true, rq.who)) return e;
  if (owns_nothing(ctx, out_stats, rq)) return SVR_OK;
  if (int e = upload_tex_table(ctx, nullptr)) return e;
  // Many objects: cull, sort and the per-object records run on the device (k_flatten.hip).  The three
  // counts of the stats then only exist after the pass (svr_get_stats); out_stats gets what the host knows.
  const size_t n_objects = n_opaque + n_transparent;
  const bool fits = n_objects <= FLATTEN_MAX_OBJECTS && ctx->meshes.size() < (1u << 20) && ctx->materials.size() < (1u << 20);
  if (fits && n_objects > 0 && (ctx->device_flatten == 1 || (ctx->device_flatten == 0 && n_objects >= 2048))) {
    PassOp in;
    in.input = PassInput::Objects;
    in.objects.reserve(n_objects);
    in.objects.insert(in.objects.end(), opaque, opaque + n_opaque);
    in.objects.insert(in.objects.end(), transparent, transparent + n_transparent);
    in.n_opaque_obj = (uint32_t)n_opaque;
    in.n_transparent_obj = (uint32_t)n_transparent;
    add_object_bounds(in.objects.data(), n_objects, &rq.n_tris, &rq.n_chunks);
    return finish_draw(ctx, SvrStats{}, out_stats, enqueue_pass(ctx, rq, std::move(in)), &t0);
  }
  return draw_objects(ctx, rq, rq.scene, opaque, n_opaque, transparent, n_transparent, out_stats, t0);
}

int svr_draw_geometry(SvrContext* ctx, const SvrSceneData* scene, const SvrRenderObject* opaque, size_t n_opaque,
                      const SvrRenderObject* transparent, size_t n_transparent, SvrStats* out_stats) {
  return draw_geometry(ctx, geometry_request("svr_draw_geometry", scene, false), opaque, n_opaque, transparent, n_transparent, out_stats);
}

int svr_draw_colored_triangle(SvrContext* ctx, SvrStats* out_stats) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (owned_tile_rows(ctx) == 0) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_colored_triangle: this context owns no tile row (svr_set_row_interleave)");
  if (int e = use_device(ctx)) return e;
  if (int e = upload_tex_table(ctx, nullptr)) return e;
  std::vector<DrawDesc> draws(1);
  std::memset(&draws[0], 0, sizeof(DrawDesc));
  draws[0].tri_count = 1;
  draws[0].flags = (uint32_t)PIPE_COLORED_TRIANGLE << F_KIND_SHIFT;
  SvrStats st{};
  st.drawcall_count = 1;
  st.triangle_count = 1;
  PassRequest rq;
  rq.who = "svr_draw_colored_triangle";
  return finish_draw(ctx, st, out_stats, run_pass(ctx, rq, draws));
}

int svr_draw_tex_image(SvrContext* ctx, SvrMesh mesh, uint32_t first_index, uint32_t index_count,
                       const float render_matrix[16], SvrImage image, SvrSampler sampler, SvrStats* out_stats) {
  if (!ctx || !render_matrix) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_tex_image: null argument");
  MeshRes* m = get_mesh(ctx, mesh);
  if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_draw_tex_image: bad mesh");
  ImageRes* im = get_image(ctx, image);
  if (!im) return fail(SVR_ERR_BAD_HANDLE, "svr_draw_tex_image: bad image");
  if (sampler == 0 || sampler > ctx->samplers.size()) return fail(SVR_ERR_BAD_HANDLE, "svr_draw_tex_image: bad sampler");
  if ((uint64_t)first_index + index_count > m->n_idx)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_tex_image: index range outside the mesh");
  if (owned_tile_rows(ctx) == 0) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_draw_tex_image: this context owns no tile row (svr_set_row_interleave)");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;  // the scratch binding slot is about to change
  TexBinding tb = make_binding(*im, ctx->samplers[sampler - 1]);
  if (int e = upload_tex_table(ctx, &tb)) return e;
  ctx->tex_slots = 0;  // scratch slot is in use: rebuild before the next mesh pass
  // a mesh record without colour factors, of kind PIPE_TEX_IMAGE, whose texture is the scratch slot
  std::vector<DrawDesc> draws(1, mesh_record(*m, render_matrix, first_index, index_count, (uint32_t)ctx->materials.size(),
                                             (uint32_t)PIPE_TEX_IMAGE << F_KIND_SHIFT));
  SvrStats st{};
  st.drawcall_count = 1;
  st.triangle_count = (int)(index_count / 3);
  PassRequest rq;
  rq.who = "svr_draw_tex_image";
  return finish_draw(ctx, st, out_stats, run_pass(ctx, rq, draws));
}

int svr_run_mesh_vert(SvrContext* ctx, SvrMesh mesh, uint32_t first_vertex, uint32_t n_vertices, const float world[16],
                      const SvrSceneData* scene, SvrMaterial material, float* out_clip, float* out_varyings) {
  if (!ctx || !world || !scene || !out_clip || !out_varyings)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_mesh_vert: null argument");
  MeshRes* m = get_mesh(ctx, mesh);
  if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_run_mesh_vert: bad mesh");
  if (material == 0 || material > ctx->materials.size()) return fail(SVR_ERR_BAD_HANDLE, "svr_run_mesh_vert: bad material");
  if ((uint64_t)first_vertex + n_vertices > m->n_vtx)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_mesh_vert: vertex range outside the mesh");
  if (n_vertices == 0) return SVR_OK;
  if (int e = use_device(ctx)) return e;
  float consts[36];
  std::memcpy(consts, world, 64);
  std::memcpy(consts + 16, scene->viewproj, 64);
  std::memcpy(consts + 32, ctx->materials[material - 1].cf, 16);
  DevPtr<float> d_consts, d_out;
  DEV_ALLOC(d_consts, sizeof(consts));
  if (dev_alloc(d_out, (size_t)n_vertices * 12 * sizeof(float)) != hipSuccess) return fail(SVR_ERR_OUT_OF_MEMORY, "svr_run_mesh_vert: hipMalloc failed");
  if (hipMemcpy(d_consts.get(), consts, sizeof(consts), hipMemcpyHostToDevice) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  float* d_clip = d_out.get();
  float* d_var = d_clip + (size_t)n_vertices * 4;
  launch_mesh_vert(m->vtx.get(), first_vertex, n_vertices, d_consts.get(), d_consts.get() + 16, d_consts.get() + 32, d_clip, d_var, ctx->stream);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(SVR_ERR_DEVICE, "mesh_vert kernel failed");
  if (hipMemcpy(out_clip, d_clip, (size_t)n_vertices * 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  if (hipMemcpy(out_varyings, d_var, (size_t)n_vertices * 32, hipMemcpyDeviceToHost) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  return SVR_OK;
}

int svr_run_vertex_shader(SvrContext* ctx, int shader, SvrMesh mesh, uint32_t first_vertex, uint32_t n_vertices,
                          const float render_matrix[16], float* out_clip, float* out_varyings) {
  if (!ctx || !out_clip || !out_varyings) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_vertex_shader: null argument");
  MeshRes* m = nullptr;
  if (shader == SVR_VS_COLORED_TRIANGLE) {
    if ((uint64_t)first_vertex + n_vertices > 3) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_vertex_shader: colored_triangle.vert has 3 vertices");
  } else if (shader == SVR_VS_COLORED_TRIANGLE_MESH) {
    if (!render_matrix) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_vertex_shader: null matrix");
    m = get_mesh(ctx, mesh);
    if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_run_vertex_shader: bad mesh");
    if ((uint64_t)first_vertex + n_vertices > m->n_vtx)
      return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_vertex_shader: vertex range outside the mesh");
  } else {
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_run_vertex_shader: unknown shader");
  }
  if (n_vertices == 0) return SVR_OK;
  if (int e = use_device(ctx)) return e;
  DevPtr<float> d_buf;  // 16 floats of matrix, then clip, then varyings
  if (dev_alloc(d_buf, (16 + (size_t)n_vertices * 12) * sizeof(float)) != hipSuccess)
    return fail(SVR_ERR_OUT_OF_MEMORY, "svr_run_vertex_shader: hipMalloc failed");
  const float zero[16] = {0};
  if (hipMemcpy(d_buf.get(), render_matrix ? render_matrix : zero, 64, hipMemcpyHostToDevice) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  float* d_clip = d_buf.get() + 16;
  float* d_var = d_clip + (size_t)n_vertices * 4;
  launch_vertex_shader(m ? m->vtx.get() : nullptr, first_vertex, n_vertices, d_buf.get(), d_clip, d_var, ctx->stream);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(SVR_ERR_DEVICE, "vertex shader kernel failed");
  if (hipMemcpy(out_clip, d_clip, (size_t)n_vertices * 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  if (hipMemcpy(out_varyings, d_var, (size_t)n_vertices * 32, hipMemcpyDeviceToHost) != hipSuccess) return fail(SVR_ERR_DEVICE, "hipMemcpy");
  return SVR_OK;
}

int svr_set_option(SvrContext* ctx, int option, int64_t value) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (option == SVR_OPT_COUNT_FRAGMENTS) {
    ctx->instrument = value != 0;
    return SVR_OK;
  }
  if (option == SVR_OPT_TUNING) {
    ctx->tuning = (uint32_t)value;
    return SVR_OK;
  }
  if (option == SVR_OPT_DEVICE_FLATTEN) {
    if (value < 0 || value > 2) return fail(SVR_ERR_INVALID_ARGUMENT, "SVR_OPT_DEVICE_FLATTEN: 0 auto, 1 always, 2 never");
    ctx->device_flatten = (int)value;
    return SVR_OK;
  }
  if (option == SVR_OPT_QUEUE_CAPS) {
    if (value < 0 || value > (1 << 30)) return fail(SVR_ERR_INVALID_ARGUMENT, "SVR_OPT_QUEUE_CAPS: out of range");
    if (int e = use_device(ctx)) return e;
    if (int e = finish_pending(ctx)) return e;
    ctx->debug_caps = (uint32_t)value;
    ctx->clip_cap = ctx->extra_cap = ctx->bin_cap = 0;  // the next pass sizes its queues afresh
    return SVR_OK;
  }
  if (option == SVR_OPT_TILE_CYCLES) {
    ctx->tile_cycles = value != 0;
    return SVR_OK;
  }
  if (option == SVR_OPT_KERNEL_TIMING) {
    if (int e = use_device(ctx)) return e;
    for (int i = 0; i < SvrContext::TRING; i++)
      if (int e = harvest_timing(ctx, i)) return e;
    ctx->acc_ms[0] = ctx->acc_ms[1] = ctx->acc_ms[2] = 0.0;
    ctx->acc_n = 0;
    ctx->kernel_timing = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    return SVR_OK;
  }
  return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_option: unknown option");
}

int svr_debug_trace_pixel(SvrContext* ctx, int x, int y) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (int e = use_device(ctx)) return e;
  if (x >= 0) {
    if (int e = finish_pending(ctx)) return e;
    if (int e = ctx->d_trace.ensure(64 * sizeof(float))) return e;
    HIPCHK(hipMemset(ctx->d_trace.p, 0, 64 * sizeof(float)));
  }
  ctx->trace_x = x;
  ctx->trace_y = y;
  return SVR_OK;
}

int svr_debug_read_trace(SvrContext* ctx, float out[64]) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_trace: null argument");
  if (!ctx->d_trace.p) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_trace: tracing was never enabled");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(out, ctx->d_trace.p, 64 * sizeof(float), hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_debug_read_bins(SvrContext* ctx, uint32_t* counts, size_t capacity, uint32_t* n_tiles) {
  if (!ctx || !n_tiles) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_bins: null argument");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  *n_tiles = ctx->last.n_tiles;
  if (!counts) return SVR_OK;
  if (capacity < 2 * (size_t)ctx->last.n_tiles || !ctx->last.tile_count)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_bins: buffer too small or no pass yet");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(counts, ctx->last.tile_count, 2 * (size_t)ctx->last.n_tiles * 4, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_debug_read_tile_cycles(SvrContext* ctx, uint32_t* cycles, size_t capacity) {
  if (!ctx || !cycles) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_tile_cycles: null argument");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  if (!ctx->last.tile_cycles || capacity < 4 * (size_t)ctx->last.n_tiles)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_tile_cycles: SVR_OPT_TILE_CYCLES was off for the last pass or buffer too small");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(cycles, ctx->last.tile_cycles, 16 * (size_t)ctx->last.n_tiles, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_get_row_costs(SvrContext* ctx, uint32_t* costs, size_t capacity, uint32_t* n_tile_rows, uint32_t* first_row, uint32_t* n_rows) {
  if (!ctx || !n_tile_rows) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_row_costs: null argument");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;  // validates whatever has finished; never waits
  *n_tile_rows = (uint32_t)ctx->row_cost.size();
  if (first_row) *first_row = ctx->row_cost_y0;
  if (n_rows) *n_rows = ctx->row_cost_rows;
  if (costs) {
    if (capacity < ctx->row_cost.size()) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_row_costs: buffer too small");
    std::memcpy(costs, ctx->row_cost.data(), ctx->row_cost.size() * sizeof(uint32_t));
  }
  return SVR_OK;
}

int svr_debug_rcp_sweep(SvrContext* ctx, int variant, uint64_t first, uint64_t count, uint64_t* mismatches, uint64_t* refined,
                        uint32_t first_bad[16]) {
  if (!ctx || !mismatches) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_rcp_sweep: null argument");
  if (variant < 0 || variant > 2 || first + count > (1ull << 32)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_rcp_sweep: bad range or variant");
  if (int e = use_device(ctx)) return e;
  DevPtr<unsigned long long> d;
  DEV_ALLOC(d, 19 * 8);
  unsigned long long h[19] = {};
  hipError_t r = hipMemset(d.get(), 0, 19 * 8);
  if (r == hipSuccess) {
    launch_rcp_sweep(variant, first, count, d.get(), ctx->stream);
    r = hipStreamSynchronize(ctx->stream);
  }
  if (r == hipSuccess) r = hipMemcpy(h, d.get(), sizeof(h), hipMemcpyDeviceToHost);
  if (r != hipSuccess) return fail(SVR_ERR_DEVICE, std::string("svr_debug_rcp_sweep: ") + hipGetErrorString(r));
  *mismatches = h[0];
  if (refined) *refined = h[1];
  if (first_bad)
    for (int k = 0; k < 16; k++) first_bad[k] = (uint32_t)h[2 + k];
  return SVR_OK;
}

int svr_sync(SvrContext* ctx) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

int svr_read_color(SvrContext* ctx, void* dst, size_t bytes, int as_rgba8) {
  if (!ctx || !dst) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_color: null argument");
  if (int e = svr_sync(ctx)) return e;
  size_t n = (size_t)ctx->W * ctx->H;
  if (ctx->fmt == SVR_COLOR_RGBA8 || !as_rgba8) {
    size_t need = n * (ctx->fmt == SVR_COLOR_RGBA8 ? 4 : 8);
    if (bytes < need) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_color: buffer too small");
    HIPCHK(hipMemcpy(dst, ctx->color, need, hipMemcpyDeviceToHost));
    return SVR_OK;
  }
  if (bytes < n * 4) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_color: buffer too small");
  if (int e = ctx->d_cvt.ensure(n * 4)) return e;
  launch_rgba16f_to_rgba8(ctx->color, ctx->d_cvt.p, (uint32_t)n, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(dst, ctx->d_cvt.p, n * 4, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_read_depth(SvrContext* ctx, float* dst, size_t bytes) {
  if (!ctx || !dst) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_depth: null argument");
  if (int e = svr_sync(ctx)) return e;
  size_t n = (size_t)ctx->W * ctx->H;
  if (bytes < n * 4) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_depth: buffer too small");
  HIPCHK(hipMemcpy(dst, ctx->depth, n * 4, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_get_stats(SvrContext* ctx, SvrStats* out) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_stats: null argument");
  if (int e = svr_sync(ctx)) return e;
  for (int i = 0; i < SvrContext::TRING; i++)
    if (int e = harvest_timing(ctx, i)) return e;
  *out = ctx->stats;
  out->replayed_passes = ctx->replayed;
  out->timed_passes = ctx->acc_n;
  if (ctx->acc_n) {
    out->geometry_ms = (float)(ctx->acc_ms[0] / ctx->acc_n);
    out->binning_ms = (float)(ctx->acc_ms[1] / ctx->acc_n);
    out->tile_ms = (float)(ctx->acc_ms[2] / ctx->acc_n);
    out->gpu_time_ms = out->geometry_ms + out->binning_ms + out->tile_ms;
  }
  return SVR_OK;
}

// ---------------------------------------------------------------- retained draw lists (include/svr_draw_list.h)
static DrawListRes* get_list(SvrContext* ctx, SvrDrawList h) {
  if (h == 0 || h > ctx->lists.size() || !ctx->lists[h - 1].alive) return nullptr;
  return &ctx->lists[h - 1];
}

// validate_object over the whole list; records the outcome against the current mesh epoch
static int check_list_objects(SvrContext* ctx, DrawListRes& L, const char* who) {
  int e = SVR_OK;
  for (size_t i = 0; i < L.objs.size() && e == SVR_OK; i++) e = validate_object(ctx, L.objs[i], i >= L.n_opaque, who);
  L.mesh_epoch = ctx->mesh_epoch;
  L.valid = e == SVR_OK;
  L.why = L.valid ? std::string() : g_err;
  return e;
}

// a new device version of the list's objects: opaque in draw order (the host path's stable sort by (material, mesh),
// over all of them — culling a subset keeps its order), then transparent; blocking copy into fresh memory, so no pass
// in flight can see it half written
static int make_list_version(const DrawListRes& L, std::shared_ptr<const ListVersion>* out) {
  auto v = std::make_shared<ListVersion>();
  const size_t n = L.objs.size();
  v->n_opaque = L.n_opaque;
  v->n_transparent = (uint32_t)(n - L.n_opaque);
  std::vector<uint32_t> order(L.n_opaque);
  std::iota(order.begin(), order.end(), 0u);
  sort_draw_order(order, L.objs.data());
  std::vector<SvrRenderObject> sorted;
  sorted.reserve(n);
  for (uint32_t i : order) sorted.push_back(L.objs[i]);
  sorted.insert(sorted.end(), L.objs.begin() + L.n_opaque, L.objs.end());
  add_object_bounds(sorted.data(), n, &v->tris_max, &v->chunks_max);
  add_object_bounds(sorted.data(), L.n_opaque, &v->tris_max_opaque, &v->chunks_max_opaque);
  if (n) {
    DEV_ALLOC(v->dev, n * sizeof(SvrRenderObject));
    HIPCHK(hipMemcpy(v->dev.get(), sorted.data(), n * sizeof(SvrRenderObject), hipMemcpyHostToDevice));
  }
  if (L.n_opaque) {  // object numbers for ID passes (include/svr_ids.h)
    for (uint32_t& i : order) i += 1u;
    DEV_ALLOC(v->obj_ids, order.size() * sizeof(uint32_t));
    HIPCHK(hipMemcpy(v->obj_ids.get(), order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  *out = std::move(v);
  return SVR_OK;
}

int svr_create_draw_list(SvrContext* ctx, const SvrRenderObject* opaque, size_t n_opaque, const SvrRenderObject* transparent,
                         size_t n_transparent, SvrDrawList* out) {
  if (!ctx || !out || (!opaque && n_opaque) || (!transparent && n_transparent))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_draw_list: null argument");
  if (n_opaque > FLATTEN_MAX_OBJECTS || n_transparent > FLATTEN_MAX_OBJECTS - n_opaque)
    return fail(SVR_ERR_UNSUPPORTED, "svr_create_draw_list: more than " + std::to_string(FLATTEN_MAX_OBJECTS) + " objects in one list");
  DrawListRes L;
  L.n_opaque = (uint32_t)n_opaque;
  L.objs.reserve(n_opaque + n_transparent);
  L.objs.insert(L.objs.end(), opaque, opaque + n_opaque);
  L.objs.insert(L.objs.end(), transparent, transparent + n_transparent);
  if (int e = check_list_objects(ctx, L, "svr_create_draw_list")) return e;
  if (int e = use_device(ctx)) return e;
  if (int e = make_list_version(L, &L.cur)) return e;
  L.alive = true;
  ctx->lists.push_back(std::move(L));
  *out = (SvrDrawList)ctx->lists.size();
  return SVR_OK;
}

int svr_update_draw_list(SvrContext* ctx, SvrDrawList list, size_t first, const SvrRenderObject* objs, size_t n) {
  if (!ctx || (!objs && n)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_update_draw_list: null argument");
  DrawListRes* L = get_list(ctx, list);
  if (!L) return fail(SVR_ERR_BAD_HANDLE, "svr_update_draw_list: bad list handle");
  if (first > L->objs.size() || n > L->objs.size() - first)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_update_draw_list: objects beyond the end of the list");
  for (size_t k = 0; k < n; k++)
    if (int e = validate_object(ctx, objs[k], first + k >= L->n_opaque, "svr_update_draw_list")) return e;
  if (n == 0) return SVR_OK;
  if (int e = use_device(ctx)) return e;
  DrawListRes next;  // copy-on-write: passes in flight keep the version they hold
  next.n_opaque = L->n_opaque;
  next.objs = L->objs;
  std::copy(objs, objs + n, next.objs.begin() + (long)first);
  if (int e = make_list_version(next, &next.cur)) return e;
  L->objs.swap(next.objs);
  L->cur = std::move(next.cur);
  (void)check_list_objects(ctx, *L, "svr_draw_list");  // objects it did not replace may still name a destroyed mesh
  return SVR_OK;
}

int svr_destroy_draw_list(SvrContext* ctx, SvrDrawList list) {
  DrawListRes* L = ctx ? get_list(ctx, list) : nullptr;
  if (!L) return fail(SVR_ERR_BAD_HANDLE, "svr_destroy_draw_list: bad list handle");
  if (int e = use_device(ctx)) return e;
  L->alive = false;
  L->cur.reset();  // the device copy goes with the last pass that holds it
  std::vector<SvrRenderObject>().swap(L->objs);
  return SVR_OK;
}

int svr_debug_read_records(SvrContext* ctx, void* draws, size_t draw_bytes, void* chunks, size_t chunk_bytes, uint32_t* n_draws,
                           uint32_t* n_chunks) {
  if (!ctx || !n_draws || !n_chunks) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_records: null argument");
  if (int e = svr_sync(ctx)) return e;
  const FrameParams& P = ctx->last;
  if (!P.draws) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_records: no pass yet");
  uint32_t nd = ctx->last_n_draws, nc = P.n_chunks;
  if (P.flatten) {  // the device knows the counts
    Counters c;
    HIPCHK(hipMemcpy(&c, P.counters, sizeof(Counters), hipMemcpyDeviceToHost));
    nd = c.flat_draws;
    nc = c.flat_chunks;
  }
  *n_draws = nd;
  *n_chunks = nc;
  if (draws) {
    if (draw_bytes < (size_t)nd * sizeof(DrawDesc)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_records: draw buffer too small");
    if (nd) HIPCHK(hipMemcpy(draws, P.draws, (size_t)nd * sizeof(DrawDesc), hipMemcpyDeviceToHost));
  }
  if (chunks) {
    if (chunk_bytes < (size_t)nc * sizeof(WaveChunk)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_records: chunk buffer too small");
    if (nc) HIPCHK(hipMemcpy(chunks, P.chunks, (size_t)nc * sizeof(WaveChunk), hipMemcpyDeviceToHost));
  }
  return SVR_OK;
}

// ---------------------------------------------------------------- multiview passes (include/svr_views.h)
// the arguments of a multiview call
struct ViewArgs {
  uint32_t n_views;
  const SvrSceneData* scenes;
  const SvrViewTargets* targets;
};

// What every multiview call checks of them, in the order of the header's refusals; completes the request: fills mv and
// makes it rq's, with the first view's scene.  A depth-only pass (include/svr_depth.h) takes no colour target and no
// clear; the views' lighting is not read, so it may differ
static int check_views(SvrContext* ctx, PassRequest& rq, const ViewArgs& va, MultiView* mv) {
  const std::string fn(rq.who);
  const SvrViewTargets* t = va.targets;
  const bool depth_only = rq.depth_only;
  if (!va.scenes || !t || (!depth_only && !t->color) || !t->depth) return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": null argument");
  if (depth_only && (t->color || t->clear_rgba))
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": a depth-only pass takes no colour target and no clear_rgba (both must be NULL)");
  if (va.n_views == 0 || va.n_views > SVR_MAX_VIEWS) return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": need 1 <= n_views <= 16");
  if ((uint64_t)va.n_views * ((ctx->H + TILE - 1) / TILE) > ROW_COST_MAX)
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": n_views * ceil(height / 32) exceeds 512 tile rows");
  if (((uintptr_t)t->color | (uintptr_t)t->depth | (uintptr_t)t->ids) & 15u)
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": targets must be 16-byte aligned");
  if (ctx->sx != 0 || ctx->sy != 0 || ctx->sw != ctx->W || ctx->sh != ctx->H)
    return fail(SVR_ERR_UNSUPPORTED, fn + ": a narrowed scissor has no multiview form");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, fn + ": interleaved rows (svr_set_row_interleave) have no multiview form");
  if (ctx->occl_bound) return fail(SVR_ERR_UNSUPPORTED, fn + ": occlusion culling (svr_set_occlusion_pyramid) has no multiview form");
  for (uint32_t k = 1; k < va.n_views && !depth_only; k++)  // one UBO: only the matrices differ between the views
    if (std::memcmp(va.scenes[k].ambient_color, va.scenes[0].ambient_color, 12 * sizeof(float)) != 0)
      return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": ambient_color, sunlight_direction and sunlight_color must be equal in every view");
  mv->n_views = va.n_views;
  mv->color = t->color;
  mv->depth = t->depth;
  mv->ids = (uint2*)t->ids;
  mv->clear = t->clear_rgba != nullptr;
  mv->packed = t->clear_rgba ? encode_clear(ctx, t->clear_rgba) : 0u;
  rq.scene = va.scenes;
  rq.mv = mv;
  return SVR_OK;
}

// svr_draw_geometry_views and svr_draw_depth_views (no transparent objects then): the host path for every view
static int draw_geometry_views(SvrContext* ctx, PassRequest rq, const ViewArgs& va, const SvrRenderObject* opaque, size_t n_opaque,
                               const SvrRenderObject* transparent, size_t n_transparent, SvrStats* out_stats) {
  if (!ctx || (!opaque && n_opaque) || (!transparent && n_transparent)) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(rq.who) + ": null argument");
  if (int e = take_depth_load_op(ctx, rq, true)) return e;
  auto t0 = std::chrono::steady_clock::now();
  MultiView mv;
  if (int e = check_views(ctx, rq, va, &mv)) return e;
  for (size_t i = 0; i < n_opaque; i++)
    if (int e = validate_object(ctx, opaque[i], false, rq.who)) return e;
  for (size_t i = 0; i < n_transparent; i++)
    if (int e = validate_object(ctx, transparent[i], true, rq.who)) return e;
  if (int e = use_device(ctx)) return e;
  if (int e = upload_tex_table(ctx, nullptr)) return e;
  return draw_objects(ctx, rq, va.scenes, opaque, n_opaque, transparent, n_transparent, out_stats, t0);
}

int svr_draw_geometry_views(SvrContext* ctx, uint32_t n_views, const SvrSceneData* scenes, const SvrViewTargets* targets,
                            const SvrRenderObject* opaque, size_t n_opaque, const SvrRenderObject* transparent, size_t n_transparent,
                            SvrStats* out_stats) {
  return draw_geometry_views(ctx, geometry_request("svr_draw_geometry_views", nullptr, false), {n_views, scenes, targets}, opaque, n_opaque,
                             transparent, n_transparent, out_stats);
}

// ---------------------------------------------------------------- drawing a retained list (include/svr_draw_list.h)
// what a multiview list call adds to a single-view one: its arguments, the MultiView made of them, and the list itself
// (its host path walks the submission-order copy)
struct ListViews {
  ViewArgs va;
  MultiView mv;
  const DrawListRes* list = nullptr;
};

// The head of the four calls that draw a list: the handle, the checks of a multiview call (views: of those), the list's
// validity — looked at again if a mesh was destroyed since — and the device.  Then the pass over the list's current
// version: `in` names it as the List input, unless the pass draws no object, and rq gets the bounds of one view (a
// depth-only pass: of the opaque objects alone, the only ones its flatten walks).
static int list_pass(SvrContext* ctx, SvrDrawList list, PassRequest& rq, ListViews* views, PassOp& in) {
  const std::string fn(rq.who);
  DrawListRes* L = get_list(ctx, list);
  if (!L) return fail(SVR_ERR_BAD_HANDLE, fn + ": bad list handle");
  if (views)
    if (int e = check_views(ctx, rq, views->va, &views->mv)) return e;
  // a mesh was destroyed since: the single-view calls have always revalidated as svr_draw_list, the others by their name
  if (L->mesh_epoch != ctx->mesh_epoch) (void)check_list_objects(ctx, *L, views ? rq.who : "svr_draw_list");
  if (!L->valid) return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": the list is no longer valid (" + L->why + ")");
  if (int e = use_device(ctx)) return e;
  const ListVersion& v = *L->cur;
  const uint32_t n_transparent = rq.depth_only ? 0u : v.n_transparent;
  if (v.n_opaque + (size_t)n_transparent > 0) {
    in.input = PassInput::List;
    in.list = L->cur;
    in.n_opaque_obj = v.n_opaque;
    in.n_transparent_obj = n_transparent;
  }
  rq.n_tris = rq.depth_only ? v.tris_max_opaque : v.tris_max;
  rq.n_chunks = rq.depth_only ? v.chunks_max_opaque : v.chunks_max;
  if (views) views->list = L;
  return SVR_OK;
}

// Per pass the host checks the handle and the mesh epoch, and enqueues the pass of svr_draw_geometry's device
// flatten with the list's current version (enqueue_pass): no per-object loop.
// svr_draw_list and svr_draw_list_depth
static int draw_list(SvrContext* ctx, SvrDrawList list, PassRequest rq, SvrStats* out_stats) {
  if (!ctx || !rq.scene) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(rq.who) + ": null argument");
  if (int e = take_depth_load_op(ctx, rq, false)) return e;
  auto t0 = std::chrono::steady_clock::now();
  PassOp in;  // no objects: svr_draw_geometry's host path, a pass of no draws
  if (int e = list_pass(ctx, list, rq, nullptr, in)) return e;
  if (owns_nothing(ctx, out_stats, rq)) return SVR_OK;
  if (int e = upload_tex_table(ctx, nullptr)) return e;
  if ((size_t)in.n_opaque_obj + in.n_transparent_obj > LIST_FUSED_MAX && (ctx->meshes.size() >= (1u << 20) || ctx->materials.size() >= (1u << 20)))
    return fail(SVR_ERR_UNSUPPORTED, std::string(rq.who) + ": lists over 4096 objects need fewer than 2^20 meshes and materials");
  return finish_draw(ctx, SvrStats{}, out_stats, enqueue_pass(ctx, rq, std::move(in)), &t0);
}

int svr_draw_list(SvrContext* ctx, SvrDrawList list, const SvrSceneData* scene, SvrStats* out_stats) {
  return draw_list(ctx, list, geometry_request("svr_draw_list", scene, false), out_stats);
}

// svr_draw_list_views and svr_draw_list_depth_views
static int draw_list_views(SvrContext* ctx, SvrDrawList list, PassRequest rq, const ViewArgs& va, SvrStats* out_stats) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(rq.who) + ": null argument");
  if (int e = take_depth_load_op(ctx, rq, true)) return e;
  auto t0 = std::chrono::steady_clock::now();
  ListViews views{va, MultiView{}, nullptr};
  PassOp in;
  if (int e = list_pass(ctx, list, rq, &views, in)) return e;
  const DrawListRes* L = views.list;
  if (int e = upload_tex_table(ctx, nullptr)) return e;
  if (in.input == PassInput::List && (size_t)in.n_opaque_obj + in.n_transparent_obj <= LIST_FUSED_MAX && ctx->device_flatten != 2) {
    // the device copy in draw order, culled and turned into records view by view by one workgroup (list_views_kernel)
    in.viewprojs.resize((size_t)va.n_views * 16);
    for (uint32_t k = 0; k < va.n_views; k++) std::memcpy(&in.viewprojs[(size_t)k * 16], va.scenes[k].viewproj, 64);
    rq.n_tris *= va.n_views;
    rq.n_chunks *= va.n_views;
    return finish_draw(ctx, SvrStats{}, out_stats, enqueue_pass(ctx, rq, std::move(in)), &t0);
  }
  // larger lists, or SVR_OPT_DEVICE_FLATTEN = 2: the host path over the list's submission-order copy
  return draw_objects(ctx, rq, va.scenes, L->objs.data(), L->n_opaque, L->objs.data() + L->n_opaque, in.n_transparent_obj, out_stats, t0);
}

int svr_draw_list_views(SvrContext* ctx, SvrDrawList list, uint32_t n_views, const SvrSceneData* scenes, const SvrViewTargets* targets,
                        SvrStats* out_stats) {
  return draw_list_views(ctx, list, geometry_request("svr_draw_list_views", nullptr, false), {n_views, scenes, targets}, out_stats);
}

// ---------------------------------------------------------------- depth-only passes (include/svr_depth.h)
int svr_draw_depth(SvrContext* ctx, const SvrSceneData* scene, const SvrRenderObject* opaque, size_t n_opaque, SvrStats* out_stats) {
  return draw_geometry(ctx, geometry_request("svr_draw_depth", scene, true), opaque, n_opaque, nullptr, 0, out_stats);
}

int svr_draw_list_depth(SvrContext* ctx, SvrDrawList list, const SvrSceneData* scene, SvrStats* out_stats) {
  return draw_list(ctx, list, geometry_request("svr_draw_list_depth", scene, true), out_stats);
}

int svr_draw_depth_views(SvrContext* ctx, uint32_t n_views, const SvrSceneData* scenes, const SvrViewTargets* targets,
                         const SvrRenderObject* opaque, size_t n_opaque, SvrStats* out_stats) {
  return draw_geometry_views(ctx, geometry_request("svr_draw_depth_views", nullptr, true), {n_views, scenes, targets}, opaque, n_opaque, nullptr, 0,
                             out_stats);
}

int svr_draw_list_depth_views(SvrContext* ctx, SvrDrawList list, uint32_t n_views, const SvrSceneData* scenes,
                              const SvrViewTargets* targets, SvrStats* out_stats) {
  return draw_list_views(ctx, list, geometry_request("svr_draw_list_depth_views", nullptr, true), {n_views, scenes, targets}, out_stats);
}

// ---------------------------------------------------------------- the ID target (include/svr_ids.h)
int svr_enable_ids(SvrContext* ctx, int on) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (int e = use_device(ctx)) return e;
  if (on) {
    if (!ctx->ids_own) {
      const size_t bytes = (size_t)ctx->W * ctx->H * sizeof(uint2);
      if (int e = finish_pending(ctx)) return e;  // the zeroing below runs outside the stream
      hipError_t r = dev_alloc(ctx->ids_own, bytes);
      if (r != hipSuccess)
        return fail(r == hipErrorOutOfMemory ? SVR_ERR_OUT_OF_MEMORY : SVR_ERR_DEVICE, std::string("svr_enable_ids: ") + hipGetErrorString(r));
      HIPCHK(hipMemset(ctx->ids_own.get(), 0, bytes));
    }
    if (!ctx->ids_bound) ctx->ids = ctx->ids_own.get();
    return SVR_OK;
  }
  if (!ctx->ids_own) return SVR_OK;
  if (int e = finish_pending(ctx)) return e;  // passes in flight (and their replays) may still write the plane
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->ids == ctx->ids_own.get()) ctx->ids = nullptr;
  ctx->ids_own.reset();
  return SVR_OK;
}

int svr_bind_id_target(SvrContext* ctx, void* ids_dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (((uintptr_t)ids_dev & 15u) != 0u) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_bind_id_target: the target must be 16-byte aligned");
  if (int e = use_device(ctx)) return e;
  // no fence: passes already enqueued carry their own ID target (also for a replay), as with svr_bind_targets
  if (int e = poll_pending(ctx)) return e;
  ctx->ids_bound = ids_dev != nullptr;
  ctx->ids = ids_dev ? (uint2*)ids_dev : ctx->ids_own.get();
  return SVR_OK;
}

int svr_get_id_target(SvrContext* ctx, void** ids_dev) {
  if (!ctx || !ids_dev) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_id_target: null argument");
  *ids_dev = ctx->ids;
  return SVR_OK;
}

int svr_read_ids(SvrContext* ctx, uint32_t* dst_host, size_t bytes) {
  if (!ctx || !dst_host) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ids: null argument");
  if (!ctx->ids) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ids: no ID target (svr_enable_ids / svr_bind_id_target)");
  const size_t n = (size_t)ctx->W * ctx->H * sizeof(uint2);
  if (bytes < n) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ids: buffer too small");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(dst_host, ctx->ids, n, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_pick(SvrContext* ctx, uint32_t x, uint32_t y, uint32_t out[2]) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_pick: null argument");
  if (x >= ctx->W || y >= ctx->H) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_pick: pixel outside the target");
  if (!ctx->ids) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_pick: no ID target (svr_enable_ids / svr_bind_id_target)");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(out, ctx->ids + (size_t)y * ctx->W + x, sizeof(uint2), hipMemcpyDeviceToHost));
  return SVR_OK;
}

// ---------------------------------------------------------------- attribute targets (include/svr_attributes.h)
namespace {
// the plane's index (bit number) of a single attribute bit, or -1
int attr_index(int attr) {
  switch (attr) {
    case SVR_ATTR_BARY: return 0;
    case SVR_ATTR_UV: return 1;
    case SVR_ATTR_NORMAL: return 2;
    case SVR_ATTR_ALBEDO: return 3;
    default: return -1;
  }
}
size_t attr_bytes(const SvrContext* ctx, int i) { return (size_t)ctx->W * ctx->H * (i == 1 ? 8u : 16u); }
}  // namespace

int svr_enable_attributes(SvrContext* ctx, uint32_t mask) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (mask & ~(uint32_t)SVR_ATTR_ALL) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_enable_attributes: unknown attribute bit");
  if (int e = use_device(ctx)) return e;
  bool change = false;
  for (int i = 0; i < 4; i++) change = change || ((mask >> i) & 1u) != (ctx->attr_own[i] ? 1u : 0u);
  if (!change) return SVR_OK;
  // the zeroing below runs outside the stream; passes in flight (and their replays) may still write a plane that goes
  if (int e = finish_pending(ctx)) return e;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  // all or nothing: the planes the mask adds are allocated and zeroed first, and a failure frees them again
  DevPtr<void> fresh[4];
  for (int i = 0; i < 4; i++) {
    if (!((mask >> i) & 1u) || ctx->attr_own[i]) continue;
    hipError_t r = dev_alloc(fresh[i], attr_bytes(ctx, i));
    if (r == hipSuccess) r = hipMemset(fresh[i].get(), 0, attr_bytes(ctx, i));
    if (r != hipSuccess)
      return fail(r == hipErrorOutOfMemory ? SVR_ERR_OUT_OF_MEMORY : SVR_ERR_DEVICE, std::string("svr_enable_attributes: ") + hipGetErrorString(r));
  }
  for (int i = 0; i < 4; i++) {
    if ((mask >> i) & 1u) {
      if (fresh[i]) ctx->attr_own[i] = std::move(fresh[i]);
      if (!ctx->attr_bound[i]) ctx->attr[i] = ctx->attr_own[i].get();
    } else if (ctx->attr_own[i]) {
      if (ctx->attr[i] == ctx->attr_own[i].get()) ctx->attr[i] = nullptr;
      ctx->attr_own[i].reset();
    }
  }
  return SVR_OK;
}

int svr_bind_attribute_target(SvrContext* ctx, int attr, void* dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  const int i = attr_index(attr);
  if (i < 0) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_bind_attribute_target: not one attribute bit");
  if (((uintptr_t)dev & 15u) != 0u) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_bind_attribute_target: the target must be 16-byte aligned");
  if (int e = use_device(ctx)) return e;
  // no fence: passes already enqueued carry their own planes (also for a replay), as with svr_bind_id_target
  if (int e = poll_pending(ctx)) return e;
  ctx->attr_bound[i] = dev != nullptr;
  ctx->attr[i] = dev ? dev : ctx->attr_own[i].get();
  return SVR_OK;
}

int svr_get_attribute_target(SvrContext* ctx, int attr, void** dev) {
  if (!ctx || !dev) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_attribute_target: null argument");
  const int i = attr_index(attr);
  if (i < 0) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_attribute_target: not one attribute bit");
  *dev = ctx->attr[i];
  return SVR_OK;
}

int svr_read_attribute(SvrContext* ctx, int attr, void* dst_host, size_t bytes) {
  if (!ctx || !dst_host) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_attribute: null argument");
  const int i = attr_index(attr);
  if (i < 0) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_attribute: not one attribute bit");
  if (!ctx->attr[i]) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_attribute: no such plane (svr_enable_attributes / svr_bind_attribute_target)");
  if (bytes != attr_bytes(ctx, i)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_attribute: the size is not the plane's");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(dst_host, ctx->attr[i], bytes, hipMemcpyDeviceToHost));
  return SVR_OK;
}

}  // extern "C"
