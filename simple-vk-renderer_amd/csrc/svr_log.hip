// svr_log.hip — a pass's submit and retirement, and the operation log with its replay (host code; no kernels here).
//
// One pass is seven kernels:
//   prologue -> setup -> clip -> count -> offsets -> fill   (internal stream: overlaps the previous tiles)
//   tiles                                                    (caller's stream, after an event)
// The pass is asynchronous like a recorded command buffer; svr_sync / read-backs are the fence.
// Per-pass device buffers only grow.  A pass whose internal queues overflowed writes nothing to the
// targets, and neither does anything after it, until the host has replayed it with larger queues
// ("the operation log" below), so results never depend on the initial capacities.
#include <algorithm>

#include "svr_context.h"

namespace svr {

// ---------------------------------------------------------------- pass machinery
// fold one finished slot of the timing ring into the running means
int harvest_timing(SvrContext* ctx, int slot) {
  if (!ctx->tev_used[slot]) return SVR_OK;
  HIPCHK(hipEventSynchronize(ctx->tev[slot][4].get()));
  const int from[3] = {0, 1, 3}, to[3] = {1, 2, 4};
  for (int k = ctx->tev_all[slot] ? 0 : 2; k < 3; k++) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->tev[slot][from[k]].get(), ctx->tev[slot][to[k]].get()));
    ctx->acc_ms[k] += ms;
  }
  ctx->acc_n++;
  ctx->tev_used[slot] = false;
  return SVR_OK;
}

namespace {

// pinned staging buffer of a log slot (free: the slot's previous operation has been retired)
int stage_buffer(SvrContext* ctx, int slot, size_t bytes, void** out) {
  if (ctx->h_stage_cap[slot] < bytes) {
    ctx->h_stage[slot].reset();
    ctx->h_stage_cap[slot] = 0;
    size_t want = bytes + bytes / 2 + 4096;
    HIPCHK_AS(pinned_alloc(ctx->h_stage[slot], want), "hipHostMalloc(&ctx->h_stage[slot], want, hipHostMallocDefault)");
    ctx->h_stage_cap[slot] = want;
  }
  *out = ctx->h_stage[slot].get();
  return SVR_OK;
}

// head of a set's tile buffer: Counters (96 B) + 80 class counters (FrameParams::cls_count) + ROW_COST_MAX row costs, then tile_count
constexpr size_t TILE_HEAD_BYTES = sizeof(Counters) + (80 + ROW_COST_MAX) * sizeof(uint32_t);
static_assert(TILE_HEAD_BYTES % 16 == 0, "tile buffer head layout");

// size the per-pass buffers for P.n_tris and the current capacities, fill the pointers
int bind_pass_buffers(SvrContext* ctx, FrameParams& P, int set_index) {
  SvrContext::PassSet& set = ctx->sets[set_index];
  if (int e = set.recs.ensure(((size_t)P.n_tris + ctx->extra_cap) * sizeof(TriRec))) return e;
  if (int e = set.clipq.ensure((size_t)ctx->clip_cap * sizeof(ClipItem))) return e;
  if (int e = set.bigq.ensure(((size_t)P.n_tris + 64) * sizeof(uint32_t))) return e;
  if (int e = set.tiles.ensure(TILE_HEAD_BYTES + ((size_t)P.n_tiles * 13 + 8 + (size_t)SPLIT_EXTRA * 8) * sizeof(uint32_t))) return e;
  if (int e = set.bins.ensure((size_t)ctx->bin_cap * sizeof(uint32_t))) return e;
  if (int e = set.pairs.ensure((size_t)ctx->bin_cap * 12)) return e;
  if (int e = set.sorta.ensure((size_t)ctx->bin_cap * 2 * sizeof(unsigned long long))) return e;
  P.recs = (TriRec*)set.recs.p;
  P.extra_cap = ctx->extra_cap;
  P.clip_queue = (ClipItem*)set.clipq.p;
  P.clip_cap = ctx->clip_cap;
  P.big_queue = (uint32_t*)set.bigq.p;
  P.counters = (Counters*)set.tiles.p;
  P.cls_count = (uint32_t*)((char*)set.tiles.p + sizeof(Counters));
  P.row_cost = P.cls_count + 80;
  P.tile_count = (uint32_t*)((char*)set.tiles.p + TILE_HEAD_BYTES);
  P.tile_offset = P.tile_count + (((size_t)P.n_tiles * 2 + 3) & ~(size_t)3);  // 16-byte aligned
  P.tile_info = (uint4*)(P.tile_offset + (((size_t)P.n_tiles * 2 + 3) & ~(size_t)3));  // 8 words per tile
  P.tile_order = (uint32_t*)P.tile_info + ((size_t)P.n_tiles + SPLIT_EXTRA) * 8;  // the quarters of split tiles head tile_info
  P.pairs = (uint2*)set.pairs.p;
  P.pair_slot = (uint32_t*)((char*)set.pairs.p + (size_t)ctx->bin_cap * 8);
  P.bins = (uint32_t*)set.bins.p;
  P.bin_cap = ctx->bin_cap;
  P.sort_arena = (unsigned long long*)set.sorta.p;
  P.sort_cap = ctx->bin_cap * 2u;  // a sorted bin needs at most twice its entries (power-of-two padding)
  P.poison = ctx->d_poison.get();
  P.host_failed_seq = ctx->h_failed_seq.get();
  return SVR_OK;
}

// Enqueue one pass.  Stage 1 (gstream): prologue (inputs + zeroing), setup, clip, bin count, offsets, bin fill
// -> ev_bin.  Stage 2 (caller's stream): wait ev_bin, tile kernel, counters to the host
// (report_kernel) -> op_done.  The caller sees stream order (everything it enqueued before the call precedes the tile
// stage, the only one that touches the targets); stage 1 depends on host inputs alone, so it overlaps
// the tile stages of the passes before it.  The op holds the pass: its parameters, number and input; op_slot: its log slot.
int submit_pass(SvrContext* ctx, const PassOp& op, int op_slot, bool pipe) {
  FrameParams P = op.P;
  const std::vector<DrawDesc>& draws = op.draws;
  const bool flatten = op.flattened(), resident = op.input == PassInput::List;
  // queue capacities: generous first guesses; overflow -> replay (recover_from_overflow)
  if (ctx->debug_caps) {  // SVR_OPT_QUEUE_CAPS: start tiny so that tests reach the replay path
    ctx->clip_cap = std::max<uint32_t>(ctx->clip_cap, ctx->debug_caps);
    ctx->extra_cap = std::max<uint32_t>(ctx->extra_cap, ctx->debug_caps);
    ctx->bin_cap = std::max<uint32_t>(ctx->bin_cap, ctx->debug_caps);
  } else {
    ctx->clip_cap = std::max<uint32_t>(ctx->clip_cap, std::max<uint32_t>(65536u, P.n_tris / 4u));
    ctx->extra_cap = std::max<uint32_t>(ctx->extra_cap, std::max<uint32_t>(65536u, P.n_tris / 2u));
    ctx->bin_cap = std::max<uint32_t>(ctx->bin_cap, std::max<uint32_t>(1u << 22, P.n_tris * 8u));
  }
  const int set_index = ctx->set_pos;
  ctx->set_pos = (ctx->set_pos + 1) % SvrContext::NSETS;
  SvrContext::PassSet& set = ctx->sets[set_index];
  // Stage 1 of a pass of few tiles (a 1920x1080 frame, a band of a sharded one) runs at the highest stream priority:
  // such a pass is bounded by stage 1 — its setup kernel finds the CUs taken by the tile kernel's first, longest
  // workgroups (21 us alone, 53 us beside it) — and with priority its workgroups get the slots that come free
  // (1080p: -5 % per frame).  A 4K frame is bounded by its tile kernel and loses 0.8 % to the same favour.
  // Either stream is made when a pass first needs it: the runtime maps a process's streams onto a handful of hardware
  // queues (four by default), and streams that share one serialise — a context that only ever renders one size of pass
  // must not take a queue it never uses (two contexts with both streams in one process: stage 1 and the tile kernel of
  // the second ended up in ONE queue, 0.093 -> 0.27 ms per 1080p frame).
  hipStream_t s = ctx->stream, g = ctx->stream;
  if (pipe) {
#ifdef SVR_AB_STAGE1_HI  // A/B builds only: stage 1 of every pass on the high-priority stream
    const bool hi = true;
#else
    const bool hi = P.n_tiles <= SPLIT_TILES_MAX;
#endif
    Stream& slot = hi ? ctx->gstream_hi : ctx->gstream;
    if (!slot) {
      hipStream_t made = nullptr;
      int least = 0, greatest = 0;
      if (hi) (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      if (!hi || hipStreamCreateWithPriority(&made, hipStreamNonBlocking, greatest) != hipSuccess) {
        if (hi) (void)hipGetLastError();  // no priorities here: an ordinary stream does the job, a little later
        made = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&made, hipStreamNonBlocking));
      }
      slot.reset(made);
    }
    g = slot.get();
  }
  if (pipe) {
    if (ctx->last_g && ctx->last_g != g) {  // keep stage 1 of consecutive passes in order across the two streams
      HIPCHK(hipEventRecord(ctx->ev_gswitch.get(), ctx->last_g));
      HIPCHK(hipStreamWaitEvent(g, ctx->ev_gswitch.get(), 0));
    }
    ctx->last_g = g;
  }
  // per-pass inputs: draws + chunks through pinned staging, one copy
  // (resident: the objects are a draw list's device copy, nothing to stage)
  const size_t n_objects = flatten ? (size_t)op.n_opaque_obj + op.n_transparent_obj : 0;
  const size_t n_views = op.viewprojs.size() / 16u;  // a multiview list pass: one draw per object and view at most
  size_t draw_bytes = (flatten ? n_objects * std::max<size_t>(n_views, 1) : draws.size()) * sizeof(DrawDesc), chunk_bytes = (size_t)P.n_chunks * sizeof(WaveChunk);
  if (int e = set.inputs.ensure(std::max<size_t>(draw_bytes + chunk_bytes + 16, 256))) return e;
  if (flatten)
    if (int e = set.flat.ensure(std::max(n_objects * (16 + sizeof(SvrRenderObject)), n_views * 64) + 128)) return e;
  if (int e = bind_pass_buffers(ctx, P, set_index)) return e;
  if (op.pyr) {  // occlusion culling (include/svr_occlusion.h)
    if (int e = set.occl.ensure(std::max<size_t>(P.n_chunks, 16))) return e;
    P.pyr = op.pyr->p.get();
    P.pyr_levels = op.pyr->levels;
    std::memcpy(P.pyr_off, op.pyr->off, sizeof(P.pyr_off));
    P.occl_flags = (uint8_t*)set.occl.p;
    // Stage 1 reads the pyramid: it waits for the last build enqueued before this pass (on the caller's stream; without
    // the pipeline, stream order does it).  The other way round needs nothing: a later build of this pyramid runs on the
    // caller's stream behind this pass's tile kernel, which waits for this pass's stage 1 (ev_bin).
    if (pipe) HIPCHK(hipStreamWaitEvent(g, op.pyr->ev_built.get(), 0));
  }
  // How far stage 1 runs ahead.  A pass of few tiles (a band of a sharded frame: stage 1 56 us, tiles 50 us) is bounded
  // by stage 1, which then wants to run back to back: it only waits for its set, last read by the tile stage of
  // NSETS passes ago (a band of an eight-way split: -16 % per frame against two sets, with the priority above).  A 4K
  // frame is bounded by its tile kernel, and stage-1 kernels that arrive earlier only take CU time from it (+0.6 %):
  // it waits for the tile stage of two passes back (which is behind that of NSETS passes ago in the stream).
  if (pipe) {
    SvrContext::PassSet& gate = P.n_tiles > SPLIT_TILES_MAX ? ctx->sets[(set_index + SvrContext::NSETS - 2) % SvrContext::NSETS] : set;
    if (gate.used) HIPCHK(hipStreamWaitEvent(g, gate.ev_tile, 0));
    else if (set.used) HIPCHK(hipStreamWaitEvent(g, set.ev_tile, 0));
  }
  void* stage = nullptr;
  if (int e = stage_buffer(ctx, op_slot, (flatten ? (resident ? n_views * 64 : n_objects * sizeof(SvrRenderObject)) : draw_bytes + chunk_bytes) + 64, &stage)) return e;
  P.host_counters = &ctx->h_counters[op_slot];
  P.host_row_cost = ctx->h_row_cost.get() + (size_t)op_slot * ROW_COST_MAX;
  P.host_clock = nullptr;
  if (op.timed) {  // (the slot is free: its previous pass has been retired)
    P.host_clock = ctx->h_clock.get() + (size_t)op_slot * CLOCK_WORDS;
    std::memset(P.host_clock, 0, sizeof(unsigned long long) * CLOCK_WORDS);
  }
  P.op_seq = op.seq;
  if (flatten) {  // the objects themselves are the input; cull, sort, draw records and chunks happen on the device
    if (!resident) std::memcpy(stage, op.objects.data(), n_objects * sizeof(SvrRenderObject));
    if (n_views) std::memcpy(stage, op.viewprojs.data(), n_views * 64);  // the prologue puts them at the head of set.flat
  } else {
    std::memcpy(stage, draws.data(), draw_bytes);
    WaveChunk* ch = reinterpret_cast<WaveChunk*>((char*)stage + draw_bytes);
    size_t ci = 0;
    for (size_t di = 0; di < draws.size(); di++)
      for (uint32_t k = 0, nk = chunk_count(draws[di].first_index, draws[di].tri_count); k < nk; k++) {
        ch[ci].draw = (uint32_t)di;
        ch[ci].first_tri = chunk_first(draws[di].first_index, k);
        ci++;
      }
  }
  P.draws = (const DrawDesc*)set.inputs.p;
  P.chunks = (const WaveChunk*)((const char*)set.inputs.p + draw_bytes);  // DrawDesc is 192 B: stays 16-byte aligned

  int ts = -1;
  if (ctx->kernel_timing >= 2) {
    ts = ctx->tev_pos;
    ctx->tev_pos = (ctx->tev_pos + 1) % SvrContext::TRING;
    if (int e = harvest_timing(ctx, ts)) return e;
    for (int k = 0; k < 5; k++)
      if (!ctx->tev[ts][k]) HIPCHK_AS(make_event(ctx->tev[ts][k], hipEventDefault), "hipEventCreate(&ctx->tev[ts][k])");
  }
  // inputs out of the staging buffer + zero the counters, class counters and tile_count (adjacent)
  launch_prologue(stage, n_views ? set.flat.p : set.inputs.p, n_views ? n_views * 64 : (flatten ? 0 : draw_bytes + chunk_bytes), P.counters,
                  TILE_HEAD_BYTES + (size_t)P.n_tiles * 2 * sizeof(uint32_t), (flatten || op.shape.multiview) ? 0u : (uint32_t)draws.size(), P.scene, g);
  if (flatten) {
    FlattenParams F;
    std::memset(&F, 0, sizeof(F));
    F.objects = resident ? op.list->dev.get() : (const SvrRenderObject*)stage;
    F.n_opaque = op.n_opaque_obj;
    F.n_transparent = op.n_transparent_obj;
    std::memcpy(F.viewproj, P.scene.viewproj, 64);
    F.meshes = (const MeshEntry*)ctx->mesh_table.p;
    F.materials = (const MatEntry*)ctx->mat_table.p;
    F.keys = (unsigned long long*)set.flat.p;
    F.draw_tris = (uint32_t*)((char*)set.flat.p + n_objects * 8);
    F.chunk_base = F.draw_tris + n_objects;
    F.objects_dev = (SvrRenderObject*)((char*)set.flat.p + ((n_objects * 16 + 63) & ~(size_t)63));
    F.draws = (DrawDesc*)set.inputs.p;
    F.chunks = (WaveChunk*)((char*)set.inputs.p + draw_bytes);
    F.counters = P.counters;
    F.ids = P.ids ? 1u : 0u;
    F.obj_ids = (P.ids && resident) ? op.list->obj_ids.get() : nullptr;
    F.n_views = (uint32_t)n_views;
    F.viewprojs = n_views ? (const float*)set.flat.p : nullptr;
    if (resident)
      launch_list_flatten(F, g);
    else
      launch_flatten(F, g);
  }
  const bool all_stages = ctx->kernel_timing >= 2;
  if (ts >= 0 && all_stages) HIPCHK(hipEventRecord(ctx->tev[ts][0].get(), g));
  launch_setup(P, op.shape.depth_only, g);
  if (ts >= 0 && all_stages) HIPCHK(hipEventRecord(ctx->tev[ts][1].get(), g));
  launch_bin_count(P, g);
  launch_bin_scan(P, g);
  launch_bin_fill(P, g, pipe ? set.ev_bin.get() : nullptr);  // ev_bin rides on the fill kernel's dispatch
  if (ts >= 0 && all_stages) HIPCHK(hipEventRecord(ctx->tev[ts][2].get(), g));
  if (pipe) HIPCHK(hipStreamWaitEvent(s, set.ev_bin.get(), 0));
  if (ts >= 0) HIPCHK(hipEventRecord(ctx->tev[ts][3].get(), s));
  // op_done rides on the pass's last kernel (a start event would be a packet of its own in front of the tile kernel:
  // with kernel timing level 1 the kernel stamps the clock itself, P.host_clock)
  launch_tiles(P, ctx->fmt, P.instrument != 0, op.shape.depth_only, s, ctx->op_done[op_slot].get());
  if (ts >= 0) {
    HIPCHK(hipEventRecord(ctx->tev[ts][4].get(), s));
    ctx->tev_used[ts] = true;
    ctx->tev_all[ts] = all_stages;
  }
  HIPCHK(hipGetLastError());
  // the one event of the pass: its counters are on the host, its set and staging buffer are free
  set.ev_tile = ctx->op_done[op_slot].get();
  set.used = true;
  ctx->last = P;
  ctx->last_n_draws = flatten ? 0u : (uint32_t)draws.size();
  return SVR_OK;
}

// what the host learns from a pass that finished without overflowing, with its counters c
int retire_pass(SvrContext* ctx, const PassOp& op, int slot, const Counters& c) {
  if (op.P.instrument) {
    ctx->stats.bin_entries = c.total_entries;
    ctx->stats.rasterized_fragments = c.rasterized;
    ctx->stats.shaded_fragments = c.shaded;
    ctx->stats.binned_triangles = c.binned;
    ctx->occl_stats.chunks_tested = c.occl_tested;
    ctx->occl_stats.chunks_culled = c.occl_culled;
    ctx->occl_stats.triangles_culled = c.occl_tris;
    if (c.hiz_bad) return fail(SVR_ERR_DEVICE, "internal check failed: the hierarchical depth test dropped a fragment that wins (" + std::to_string(c.hiz_bad) + ")");
  }
  if (op.flattened()) {  // device-flattened passes learn these late
    ctx->stats.drawcall_count = (int32_t)c.flat_draws;
    ctx->stats.triangle_count = (int32_t)c.flat_tris;
    ctx->stats.culled_draws = c.flat_culled;
  }
  // the tile rows' costs (posted by its tile kernel before anything else): svr_get_row_costs, of single-view colour passes
  if (op.shape.multiview || op.shape.depth_only) return SVR_OK;
  const uint32_t* src = ctx->h_row_cost.get() + (size_t)slot * ROW_COST_MAX;
  ctx->row_cost.assign(src, src + std::min<uint32_t>(op.P.tiles_y, ROW_COST_MAX));
  ctx->row_cost_y0 = op.P.sy;
  ctx->row_cost_rows = op.P.sh;
  return SVR_OK;
}

}  // namespace

// ---------------------------------------------------------------- the operation log
// Passes run asynchronously and several deep, so the host learns of a queue overflow late.  The
// guarantee "results never depend on queue capacities" is kept like this: the tile kernel of a pass
// that overflowed writes nothing and raises a sticky device flag (poison); every later target-writing
// kernel of this context (of a pass or of any other logged operation) sees the flag and writes nothing either, so the
// targets freeze in the state before the failed pass.  The host keeps every target-writing operation
// in a log until its completion event has fired and its counters were checked; on an overflow it
// drains the device, lowers the flag, grows the queues and replays the log from the failed operation
// on, in order.  (Work the caller itself enqueues between passes is not in the log; SvrStats.
// replayed_passes tells such a caller that a replay happened — see dist.py.)
// Of the operations only a pass records an event of its own (an event between two kernels is a bubble in the stream)
// and has queues that can overflow.  Every other kind is one submit function: it writes nothing while the poison flag
// is up, and a replay runs it again as it was.
static int launched() {
  HIPCHK(hipGetLastError());
  return SVR_OK;
}
int submit(SvrContext* ctx, const ClearOp& op, int, bool) {
  const size_t px_bytes = op.fmt == SVR_COLOR_RGBA16F ? 8 : 4;
  launch_fill_color((char*)op.target + (size_t)op.y_first * op.row_width * px_bytes, op.row_width * op.n_rows, op.fmt, op.packed, ctx->d_poison.get(),
                    ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const BackgroundOp& op, int, bool) {
  launch_background(op.target, op.fmt, op.w, op.h, op.y_first, op.n_rows, op.effect, op.data, ctx->d_poison.get(), ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const BlitOp& op, int, bool replaying) {
  launch_blit(op.src, op.src_fmt, op.src_w, op.src_h, op.dst, op.dst_w, op.dst_h, op.y_first, op.n_rows, op.dst_fmt, ctx->d_poison.get(), op.rstride,
              op.roff, op.row_end, op.status, replaying ? 2u : 0u, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const PyramidOp& op, int, bool) {
  launch_pyramid(op.src, op.W, op.H, op.pyr->p.get(), op.pyr->off, op.pyr->levels, ctx->d_poison.get(), ctx->stream);
  HIPCHK(hipEventRecord(op.pyr->ev_built.get(), ctx->stream));
  return launched();
}
int submit(SvrContext* ctx, const LightOp& op, int slot, bool) {
  if (!op.lights.empty()) {  // (the slot's staging buffer is free: its previous operation has been retired)
    const size_t bytes = op.lights.size() * sizeof(SvrPointLight);
    void* stage = nullptr;
    if (int e = stage_buffer(ctx, slot, bytes, &stage)) return e;
    std::memcpy(stage, op.lights.data(), bytes);
    HIPCHK(hipMemcpyAsync(ctx->d_lights.get(), stage, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  launch_light(op.launch, op.color_fmt, op.tiles_y, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const PostOp& op, int, bool) {
  launch_post(op, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const TemporalOp& op, int, bool) {
  launch_temporal(op, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const AmbientOp& op, int, bool) {
  launch_ambient(op, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const ExposureOp& op, int, bool) {
  launch_exposure(op, ctx->stream);
  return launched();
}
// One copy through the slot's staging buffer: the statistics {submitted, 0, 0, -}, then the commands, the texture table,
// the vertices and the indices, each on 16 bytes.  The device buffers only grow; growing frees the old one, which waits
// for the device, so an overlay still in flight has finished with it.
int submit(SvrContext* ctx, const OverlayOp& op, int slot, bool) {
  auto up16 = [](size_t n) { return (n + 15u) & ~(size_t)15u; };
  const size_t o_cmds = 16, o_tex = o_cmds + up16(op.cmds.size() * sizeof(OverlayCmdDev));
  const size_t o_vtx = o_tex + up16(op.textures.size() * sizeof(SvrOverlayTexture));
  const size_t o_idx = o_vtx + up16(op.vertices.size() * sizeof(SvrOverlayVertex));
  const size_t bytes = o_idx + up16(op.indices.size() * sizeof(uint16_t));
  void* stage = nullptr;
  if (int e = stage_buffer(ctx, slot, bytes, &stage)) return e;
  if (int e = ctx->d_overlay_in.ensure(bytes)) return e;
  const size_t box_bytes = up16((size_t)op.launch.n_tris * sizeof(uint2));
  if (int e = ctx->d_overlay_recs.ensure(box_bytes + (size_t)op.launch.n_tris * OVERLAY_REC_WORDS * sizeof(uint32_t))) return e;
  char* h = static_cast<char*>(stage);
  const uint32_t head[4] = {op.submitted, 0u, 0u, 0u};
  std::memcpy(h, head, sizeof(head));
  std::memcpy(h + o_cmds, op.cmds.data(), op.cmds.size() * sizeof(OverlayCmdDev));
  std::memcpy(h + o_tex, op.textures.data(), op.textures.size() * sizeof(SvrOverlayTexture));
  std::memcpy(h + o_vtx, op.vertices.data(), op.vertices.size() * sizeof(SvrOverlayVertex));
  std::memcpy(h + o_idx, op.indices.data(), op.indices.size() * sizeof(uint16_t));
  char* d = static_cast<char*>(ctx->d_overlay_in.p);
  HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
  OverlayLaunch L = op.launch;
  L.stats = reinterpret_cast<uint32_t*>(d);
  L.cmds = reinterpret_cast<const OverlayCmdDev*>(d + o_cmds);
  L.textures = reinterpret_cast<const SvrOverlayTexture*>(d + o_tex);
  L.vertices = reinterpret_cast<const SvrOverlayVertex*>(d + o_vtx);
  L.indices = reinterpret_cast<const uint16_t*>(d + o_idx);
  L.boxes = static_cast<uint2*>(ctx->d_overlay_recs.p);
  L.recs = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->d_overlay_recs.p) + box_bytes);
  launch_overlay(L, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const UpscaleOp& op, int, bool replaying) {
  launch_upscale(op, replaying ? 2u : 0u, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const FogOp& op, int, bool) {
  launch_fog(op.launch, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const DofOp& op, int, bool) {
  launch_dof(op.launch, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const MotionOp& op, int, bool) {
  launch_motion(op.launch, ctx->stream);
  return launched();
}
int submit(SvrContext* ctx, const ReflectOp& op, int, bool) {
  launch_reflect(op.launch, ctx->stream);
  return launched();
}

namespace {

// One operation of the log again, behind a lowered flag.  An operation without queues of its own: as it was.
template <class Op> int replay(SvrContext* ctx, const Op& op, int slot, uint32_t) {
  HIPCHK(hipMemsetAsync(ctx->d_poison.get(), 0, sizeof(uint32_t), ctx->stream));
  return submit(ctx, op, slot, true);
}
// A pass: without the pipeline, with queues grown until it fits
int replay(SvrContext* ctx, const PassOp& op, int slot, uint32_t failed_seq) {
  bool done = false;
  Counters c;
  std::memset(&c, 0, sizeof(c));
  // the pass that failed reported its counters with its number (tile_kernel): grow before the first replay.
  // The passes behind it were only void, not known to overflow: they start from the capacities as they are.
  if (op.seq == failed_seq && ctx->h_counters[slot].overflow) c = ctx->h_counters[slot];
  for (int attempt = 0; attempt < 13 && !done; attempt++) {
    if (c.overflow & 1u) ctx->clip_cap = std::max<uint32_t>(ctx->clip_cap * 2u, c.n_clip + 1024u);
    if (c.overflow & 2u) ctx->extra_cap = std::max<uint32_t>(ctx->extra_cap * 2u, c.n_extra + 1024u);
    if (c.overflow & 4u) {
      uint32_t need = std::max(c.total_entries, c.n_pairs + c.n_pairs_rest);
      ctx->bin_cap = std::max<uint32_t>(ctx->bin_cap * 2u, need + need / 4u);
    }
    HIPCHK(hipMemsetAsync(ctx->d_poison.get(), 0, sizeof(uint32_t), ctx->stream));
    if (int e = submit_pass(ctx, op, slot, false)) return e;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(&c, ctx->last.counters, sizeof(Counters), hipMemcpyDeviceToHost));
    *ctx->h_failed_seq = 0;
    done = c.overflow == 0;
  }
  if (!done) return fail(SVR_ERR_OVERFLOW, "a pass kept overflowing its internal queues after 12 replays");
  if (int e = retire_pass(ctx, op, slot, c)) return e;
  ctx->replayed++;
  return SVR_OK;
}

int recover_from_overflow(SvrContext* ctx) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->gstream) HIPCHK(hipStreamSynchronize(ctx->gstream.get()));
  if (ctx->gstream_hi) HIPCHK(hipStreamSynchronize(ctx->gstream_hi.get()));
  const uint32_t failed_seq = *(volatile uint32_t*)ctx->h_failed_seq.get();
  *ctx->h_failed_seq = 0;
  for (const LoggedOp& op : ctx->log) {
    const int e = std::visit([&](const auto& what) { return replay(ctx, what, op.slot, failed_seq); }, op.what);
    if (e == SVR_ERR_OVERFLOW) ctx->log.clear();  // the pass does not fit: nothing of the log is tried again
    if (e) return e;
  }
  HIPCHK(hipMemsetAsync(ctx->d_poison.get(), 0, sizeof(uint32_t), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->log.clear();
  return SVR_OK;
}

}  // namespace

// validate finished operations front to back; blocking = wait for all of them (a fence).
// An operation without an event of its own is done when a pass behind it is, or when the stream has drained.
int retire_ops(SvrContext* ctx, bool blocking) {
  while (!ctx->log.empty()) {
    size_t k = 0;  // first pass at or behind the front
    while (k < ctx->log.size() && !ctx->log[k].as_pass()) k++;
    if (k == ctx->log.size()) {  // only operations without an event of their own left
      if (!blocking) return SVR_OK;
      HIPCHK(hipStreamSynchronize(ctx->stream));
      ctx->log.clear();
      return SVR_OK;
    }
    const int slot = ctx->log[k].slot;
    const PassOp& pass = *ctx->log[k].as_pass();
    if (blocking) {
      HIPCHK(hipEventSynchronize(ctx->op_done[slot].get()));
    } else {
      hipError_t q = hipEventQuery(ctx->op_done[slot].get());
      if (q == hipErrorNotReady) return SVR_OK;
      HIPCHK(q);
    }
    // the device names the first pass that overflowed (tile_kernel); everything from it on is void
    const uint32_t failed = *(volatile uint32_t*)ctx->h_failed_seq.get();
    if (failed != 0 && failed == pass.seq) {
      // the operations in front of the failed pass did land: only it and what follows is replayed
      ctx->log.erase(ctx->log.begin(), ctx->log.begin() + (long)k);
      return recover_from_overflow(ctx);
    }
    if (pass.timed) {  // the kernel's own stamps of the 100 MHz wall clock: first workgroup's start, last workgroup's end
      const volatile unsigned long long* w = ctx->h_clock.get() + (size_t)slot * CLOCK_WORDS;
      unsigned long long t_end = 0;
      const unsigned long long t_start = w[0];
      for (uint32_t i = 1; i <= 64; i++) {
        const unsigned long long t = w[i * CLOCK_STRIDE];
        if (t > t_end) t_end = t;
      }
      if (t_start != 0 && t_end >= t_start) {  // (a void pass stamps too; a pass whose kernel never ran does not count)
        ctx->acc_ms[2] += (double)(t_end - t_start) * 1e-5;
        ctx->acc_n++;
      }
    }
    const int e = retire_pass(ctx, pass, slot, ctx->h_counters[slot]);
    ctx->log.erase(ctx->log.begin(), ctx->log.begin() + (long)k + 1);
    if (e) return e;
  }
  return SVR_OK;
}

// A slot's staging buffer, counters and event are free once its previous operation has retired.  With the log full, the
// oldest pass is waited for; a log of operations without an event of their own drains the stream.
int log_slot(SvrContext* ctx, int* slot) {
  if ((int)ctx->log.size() >= SvrContext::MAX_OPS) {
    if (int e = retire_ops(ctx, false)) return e;
    if ((int)ctx->log.size() >= SvrContext::MAX_OPS) {
      const auto oldest_pass = std::find_if(ctx->log.begin(), ctx->log.end(), [](const LoggedOp& op) { return op.as_pass() != nullptr; });
      if (oldest_pass != ctx->log.end()) {
        HIPCHK(hipEventSynchronize(ctx->op_done[oldest_pass->slot].get()));
        if (int e = retire_ops(ctx, false)) return e;
      } else if (int e = retire_ops(ctx, true)) {
        return e;
      }
    }
  }
  *slot = ctx->op_pos;
  ctx->op_pos = (ctx->op_pos + 1) % SvrContext::MAX_OPS;
  return SVR_OK;
}

int log_pass(SvrContext* ctx, PassOp&& pass) {
  int slot = 0;
  if (int e = log_slot(ctx, &slot)) return e;
  pass.seq = ctx->next_seq++;
  if (ctx->next_seq == 0) ctx->next_seq = 1;
  pass.timed = ctx->kernel_timing == 1;
  ctx->log.emplace_back(slot, std::move(pass));
  std::memset(&ctx->h_counters[slot], 0, sizeof(Counters));
  const int e = submit_pass(ctx, *ctx->log.back().as_pass(), slot, !(ctx->tuning & TUNE_NO_PIPELINE));
  if (e) ctx->log.pop_back();
  return e;
}

// A clear of whole scissor rows is not run when it is asked for: the pass that follows writes every
// pixel of those rows anyway (its tile grid covers the scissor), so it takes the clear value for the
// pixels it does not cover and the separate 8-bytes-per-pixel fill disappears — what a Vulkan renderer
// gets from loadOp = CLEAR instead of a clear command.  Anything else that touches or exposes the
// target first (another operation, a read-back, a fence, a change of targets) runs the clear as its
// own kernel here.  SVR_OPT_TUNING bit 2 turns the deferral off.
int flush_clear(SvrContext* ctx) {
  if (!ctx->pending_clear.valid) return SVR_OK;
  const SvrContext::PendingClear pc = ctx->pending_clear;
  ctx->pending_clear.valid = false;
  return log_op(ctx, ClearOp{pc.target, pc.fmt, ctx->W, pc.y0, pc.rows, pc.packed});
}

int finish_pending(SvrContext* ctx) {  // the fence
  if (int e = flush_clear(ctx)) return e;
  return retire_ops(ctx, true);
}
int poll_pending(SvrContext* ctx) { return (ctx->tuning & TUNE_NO_POLL) ? SVR_OK : retire_ops(ctx, false); }

}  // namespace svr
