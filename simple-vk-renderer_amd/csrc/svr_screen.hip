// svr_screen.hip — the operations over finished targets (host code; no kernels here): the depth pyramid and occlusion
// culling's calls, the deferred lighting pass, the HDR post pass, the fog pass, the depth of field pass, the motion blur pass, the reflection pass, auto-exposure,
// temporal antialiasing, ambient occlusion, the UI overlay and the upscaled present, with their targets and read-backs.
// Each validates its arguments, allocates what its first call needs, records its kernels' parameters in a payload of
// its kind and logs it (svr_context.h, svr_log.hip).
#include <cmath>
#include <cstddef>

#include "svr_context.h"
#include "svr_overlay_font.h"

using namespace svr;

extern "C" {

// ---------------------------------------------------------------- what several passes check and fill alike
// the shadow map a pass was handed (C18), as its kernels read it; depth == null: none, and S stays empty
static int shadow_map(const char* who, const float* depth, uint32_t w, uint32_t h, const float* viewproj, float bias, ShadowMap& S) {
  S = ShadowMap{};
  if (!depth) return SVR_OK;
  if (w == 0 || h == 0 || w > (1u << 24) || h > (1u << 24))
    return fail(SVR_ERR_INVALID_ARGUMENT, std::string(who) + ": the shadow map's extent must be 1 .. 2^24 each way");
  S.depth = depth;
  S.w = w;
  S.h = h;
  S.half_w = (float)w * 0.5f;
  S.half_h = (float)h * 0.5f;
  std::memcpy(S.viewproj, viewproj, sizeof(S.viewproj));
  S.bias = bias;
  return SVR_OK;
}

// a matrix a pass divides by: 16 finite floats
static int finite_matrix(const char* who, const char* name, const float* m) {
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(m[i])) return fail(SVR_ERR_INVALID_ARGUMENT, std::string(who) + ": " + name + "[" + std::to_string(i) + "] is not finite");
  return SVR_OK;
}

// ---------------------------------------------------------------- occlusion culling (include/svr_occlusion.h)
static std::shared_ptr<PyramidMem> get_pyramid(SvrContext* ctx, SvrDepthPyramid h) {
  if (h == 0 || h > ctx->pyramids.size()) return nullptr;
  return ctx->pyramids[h - 1];
}

int svr_create_depth_pyramid(SvrContext* ctx, SvrDepthPyramid* out) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_create_depth_pyramid: null argument");
  if (int e = use_device(ctx)) return e;
  auto m = std::make_shared<PyramidMem>();
  m->levels = pyramid_levels(ctx->W, ctx->H);
  m->words = pyramid_offsets(ctx->W, ctx->H, m->off);
  DEV_ALLOC(m->p, m->words * sizeof(uint32_t));
  HIPCHK_AS(make_event(m->ev_built, hipEventDisableTiming), "hipEventCreateWithFlags(&m->ev_built, hipEventDisableTiming)");
  // all texels 0.0 until the first build: a pass culls nothing against it
  HIPCHK(hipMemsetAsync(m->p.get(), 0, m->words * sizeof(uint32_t), ctx->stream));
  HIPCHK(hipEventRecord(m->ev_built.get(), ctx->stream));
  ctx->pyramids.push_back(m);
  *out = (SvrDepthPyramid)ctx->pyramids.size();
  return SVR_OK;
}

int svr_destroy_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_destroy_depth_pyramid: null context");
  if (!get_pyramid(ctx, pyr)) return fail(SVR_ERR_BAD_HANDLE, "svr_destroy_depth_pyramid: bad pyramid handle");
  if (int e = use_device(ctx)) return e;
  ctx->pyramids[pyr - 1].reset();  // the memory goes with the last logged operation that holds it
  if (ctx->occl_bound == pyr) ctx->occl_bound = 0;
  return SVR_OK;
}

int svr_build_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr, const float* depth_dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_build_depth_pyramid: null context");
  std::shared_ptr<PyramidMem> m = get_pyramid(ctx, pyr);
  if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_build_depth_pyramid: bad pyramid handle");
  const float* src = depth_dev ? depth_dev : ctx->depth;
  if (!src) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_build_depth_pyramid: no depth target");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  return log_op(ctx, PyramidOp{std::move(m), src, ctx->W, ctx->H});
}

int svr_set_occlusion_pyramid(SvrContext* ctx, SvrDepthPyramid pyr) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_occlusion_pyramid: null context");
  if (pyr != 0 && !get_pyramid(ctx, pyr)) return fail(SVR_ERR_BAD_HANDLE, "svr_set_occlusion_pyramid: bad pyramid handle");
  ctx->occl_bound = pyr;
  return SVR_OK;
}

int svr_read_depth_pyramid(SvrContext* ctx, SvrDepthPyramid pyr, uint32_t level, void* dst, size_t bytes, uint32_t* n_levels) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_depth_pyramid: null context");
  std::shared_ptr<PyramidMem> m = get_pyramid(ctx, pyr);
  if (!m) return fail(SVR_ERR_BAD_HANDLE, "svr_read_depth_pyramid: bad pyramid handle");
  if (n_levels) *n_levels = m->levels;
  if (level < 1 || level > m->levels)
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_depth_pyramid: level out of range (1.." + std::to_string(m->levels) + ")");
  const size_t need = (size_t)(((ctx->W - 1u) >> level) + 1u) * (((ctx->H - 1u) >> level) + 1u) * sizeof(uint32_t);
  if (!dst || bytes < need) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_depth_pyramid: destination too small");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(dst, m->p.get() + m->off[level], need, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_get_occlusion_stats(SvrContext* ctx, SvrOcclusionStats* out) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_occlusion_stats: null argument");
  if (int e = svr_sync(ctx)) return e;
  *out = ctx->occl_stats;
  return SVR_OK;
}

int svr_debug_read_occlusion(SvrContext* ctx, uint32_t* bits, size_t capacity, uint32_t* n_chunks) {
  if (!ctx || !n_chunks) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_occlusion: null argument");
  if (int e = svr_sync(ctx)) return e;
  const FrameParams& P = ctx->last;
  if (!P.draws) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_occlusion: no pass yet");
  uint32_t nc = P.n_chunks;
  if (P.flatten) {  // the device knows the count
    Counters c;
    HIPCHK(hipMemcpy(&c, P.counters, sizeof(Counters), hipMemcpyDeviceToHost));
    nc = c.flat_chunks;
  }
  *n_chunks = nc;
  if (!bits) return SVR_OK;
  if (capacity < ((size_t)nc + 31u) / 32u) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_occlusion: bit buffer too small");
  std::vector<uint8_t> flags(nc, 0);
  if (P.occl_flags && nc) HIPCHK(hipMemcpy(flags.data(), P.occl_flags, nc, hipMemcpyDeviceToHost));
  std::memset(bits, 0, ((size_t)nc + 31u) / 32u * sizeof(uint32_t));
  for (uint32_t i = 0; i < nc; i++)
    if (flags[i]) bits[i / 32u] |= 1u << (i % 32u);
  return SVR_OK;
}
// ---------------------------------------------------------------- the deferred lighting pass (include/svr_lighting.h)
int svr_light_pass(SvrContext* ctx, const SvrLightPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: null argument");
  if (pass->n_lights > SVR_MAX_LIGHTS) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: more than SVR_MAX_LIGHTS lights");
  if (pass->n_lights && !pass->lights) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: null light array");
  for (uint32_t i = 0; i < pass->n_lights; i++)
    if (!(std::isfinite(pass->lights[i].radius) && pass->lights[i].radius > 0.0f))
      return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: light " + std::to_string(i) + ": the radius must be finite and greater than 0");
  ShadowMap shadow;
  if (int e = shadow_map("svr_light_pass", pass->shadow_depth, pass->shadow_width, pass->shadow_height, pass->shadow_viewproj, pass->shadow_bias, shadow)) return e;
  if (!ctx->attr[2] || !ctx->attr[3])
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: needs the SVR_ATTR_NORMAL and SVR_ATTR_ALBEDO planes (svr_enable_attributes / svr_bind_attribute_target)");
  const float* ao = nullptr;  // include/svr_ambient.h: the ambient target current at this call
  if (ctx->light_ao) {
    ao = ctx->ambient_bound ? ctx->ambient_bound : ctx->d_ambient_own.get();
    if (!ao) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_light_pass: svr_set_light_ambient_occlusion is on and there is no ambient target (svr_ambient_pass / svr_bind_ambient_target)");
  }
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  if (!ctx->d_lights) DEV_ALLOC(ctx->d_lights, SVR_MAX_LIGHTS * sizeof(SvrPointLight));
  if (!ctx->d_light_tiles) DEV_ALLOC(ctx->d_light_tiles, (size_t)((ctx->W + TILE - 1) / TILE) * ((ctx->H + TILE - 1) / TILE) * sizeof(uint32_t));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  LightOp op;
  op.color_fmt = ctx->fmt;
  op.lights.assign(pass->lights, pass->lights + pass->n_lights);
  op.tiles_y = owned_tile_rows(ctx);
  LightLaunch& L = op.launch;
  L.color = ctx->color;
  L.depth = ctx->depth;
  L.normal = (const float4*)ctx->attr[2];
  L.albedo = (const float4*)ctx->attr[3];
  L.W = ctx->W;
  L.H = ctx->H;
  L.sx = ctx->sx;
  L.sy = ctx->sy;
  L.sw = ctx->sw;
  L.sh = ctx->sh;
  L.tiles_x = (ctx->sw + TILE - 1) / TILE;
  L.rstride = ctx->rstride;
  L.roff = ctx->roff;
  L.two_over_w = 2.0f / (float)ctx->W;
  L.two_over_h = 2.0f / (float)ctx->H;
  std::memcpy(L.inv_viewproj, pass->inv_viewproj, sizeof(L.inv_viewproj));
  std::memcpy(L.ambient_color, pass->ambient_color, sizeof(L.ambient_color));
  std::memcpy(L.sunlight_direction, pass->sunlight_direction, sizeof(L.sunlight_direction));
  std::memcpy(L.sunlight_color, pass->sunlight_color, sizeof(L.sunlight_color));
  L.lights = ctx->d_lights.get();
  L.n_lights = pass->n_lights;
  L.shadow = shadow;
  L.tile_counts = ctx->d_light_tiles.get();
  L.poison = ctx->d_poison.get();
  L.ao = ao;
  const uint32_t n_tiles = L.tiles_x * op.tiles_y;
  if (int e = log_op(ctx, std::move(op))) return e;
  ctx->light_tiles_n = n_tiles;
  return SVR_OK;
}

int svr_debug_read_light_tiles(SvrContext* ctx, uint32_t* counts, size_t capacity, uint32_t* n_tiles) {
  if (!ctx || !n_tiles) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_light_tiles: null argument");
  if (int e = svr_sync(ctx)) return e;
  *n_tiles = ctx->light_tiles_n;
  if (!counts) return SVR_OK;
  if (!ctx->d_light_tiles) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_light_tiles: no lighting pass yet");
  if (capacity < ctx->light_tiles_n) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_light_tiles: buffer too small");
  if (ctx->light_tiles_n) HIPCHK(hipMemcpy(counts, ctx->d_light_tiles.get(), (size_t)ctx->light_tiles_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SVR_OK;
}

// ---------------------------------------------------------------- the HDR post pass (include/svr_post.h)
static int exposure_memory(SvrContext* ctx);  // include/svr_exposure.h, below

int svr_post_pass(SvrContext* ctx, const SvrPostPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: null argument");
  if (!(std::isfinite(pass->exposure) && pass->exposure > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: the exposure must be finite and greater than 0");
  if (!(std::isfinite(pass->bloom_threshold) && pass->bloom_threshold >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: the bloom threshold must be finite and at least 0");
  if (!(std::isfinite(pass->bloom_intensity) && pass->bloom_intensity >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: the bloom intensity must be finite and at least 0");
  if (pass->bloom_levels > SVR_POST_MAX_LEVELS) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: more than SVR_POST_MAX_LEVELS bloom levels");
  if (pass->tonemap > SVR_TONEMAP_ACES) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_post_pass: unknown tone-mapping operator");
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_post_pass: the colour target must be RGBA16F (an RGBA8 target holds no HDR values)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_post_pass: not under svr_set_row_interleave with a stride above 1");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  uint32_t off[SVR_POST_MAX_LEVELS], lw[SVR_POST_MAX_LEVELS], lh[SVR_POST_MAX_LEVELS];
  // (the extents grow with the image's, so the levels of any scissor fit in those of the whole target)
  if (!ctx->d_post_levels) DEV_ALLOC(ctx->d_post_levels, post_level_layout(ctx->W, ctx->H, SVR_POST_MAX_LEVELS, off, lw, lh) * sizeof(uint2));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  PostOp P{};
  P.color = (uint2*)ctx->color;
  P.W = ctx->W;
  P.sx = ctx->sx;
  P.sy = ctx->sy;
  P.sw = ctx->sw;
  P.sh = ctx->sh;
  P.levels = ctx->d_post_levels.get();
  P.n_levels = pass->bloom_levels;
  post_level_layout(ctx->sw, ctx->sh, pass->bloom_levels, P.off, P.lw, P.lh);
  P.exposure = pass->exposure;
  P.threshold = pass->bloom_threshold;
  P.intensity = pass->bloom_intensity;
  P.tonemap = pass->tonemap;
  P.poison = ctx->d_poison.get();
  if (ctx->post_auto) {  // include/svr_exposure.h: e = exposure * the state's, formed on the device
    if (int e = exposure_memory(ctx)) return e;
    P.auto_exposure = reinterpret_cast<const float*>(ctx->d_exposure.get());  // SvrExposureState::exposure is the first word
  }
  return log_op(ctx, std::move(P));
}

// ---------------------------------------------------------------- the fog pass (include/svr_fog.h)
static_assert(sizeof(SvrFogPass) == 232 && offsetof(SvrFogPass, shadow_depth) == 144 && offsetof(SvrFogPass, frame_index) == 228, "include/svr_fog.h");

int svr_fog_pass(SvrContext* ctx, const SvrFogPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: null argument");
  if (!(std::isfinite(pass->density) && pass->density >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: the density must be finite and at least 0");
  if (!(std::isfinite(pass->height_falloff) && pass->height_falloff >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: the height falloff must be finite and at least 0");
  if (!(std::isfinite(pass->max_distance) && pass->max_distance > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: max_distance must be finite and greater than 0");
  if (pass->steps < 1u || pass->steps > SVR_FOG_MAX_STEPS) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: steps must be in 1..SVR_FOG_MAX_STEPS");
  if (!(std::fabs(pass->anisotropy) < 1.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: the anisotropy must be greater than -1 and less than 1");
  if (!(std::isfinite(pass->edge_sharpness) && pass->edge_sharpness >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_fog_pass: the edge sharpness must be finite and at least 0");
  ShadowMap shadow;
  if (int e = shadow_map("svr_fog_pass", pass->shadow_depth, pass->shadow_width, pass->shadow_height, pass->shadow_viewproj, pass->shadow_bias, shadow)) return e;
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_fog_pass: the colour target must be RGBA16F (the pass works in scene-linear HDR)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_fog_pass: not under svr_set_row_interleave with a stride above 1");
  if (pass->density == 0.0f) return SVR_OK;  // no medium: the target keeps its bits, and no kernel is enqueued to rewrite them
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  // (the grid's extents grow with the image's, so the blocks of any scissor fit in those of the whole target)
  const size_t cap = fog_blocks(ctx->W, ctx->H);
  if (!ctx->d_fog) DEV_ALLOC(ctx->d_fog, cap * (sizeof(float4) + sizeof(float)));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  FogOp op;
  FogLaunch& F = op.launch;
  F.color = (uint2*)ctx->color;
  F.depth = ctx->depth;
  F.W = ctx->W;
  F.sx = ctx->sx;
  F.sy = ctx->sy;
  F.sw = ctx->sw;
  F.sh = ctx->sh;
  F.gw = (ctx->sw + 1u) / 2u;
  F.gh = (ctx->sh + 1u) / 2u;
  F.st = ctx->d_fog.get();
  F.te = reinterpret_cast<float*>(ctx->d_fog.get() + cap);
  F.two_over_w = 2.0f / (float)ctx->W;
  F.two_over_h = 2.0f / (float)ctx->H;
  std::memcpy(F.inv_viewproj, pass->inv_viewproj, sizeof(F.inv_viewproj));
  std::memcpy(F.cam, pass->camera_position, sizeof(F.cam));
  F.density = pass->density;
  F.kh = pass->height_falloff * 0x1.715476p+0f;  // C57
  F.height_base = pass->height_base;
  F.max_distance = pass->max_distance;
  F.steps = pass->steps;
  std::memcpy(F.fog_color, pass->fog_color, sizeof(F.fog_color));
  std::memcpy(F.sun_color, pass->sun_color, sizeof(F.sun_color));
  {  // C58: L / |L|, and the phase function's constants
    const float* L = pass->sunlight_direction;
    const float l2 = std::fma(L[2], L[2], std::fma(L[1], L[1], L[0] * L[0]));
    const float inv = (std::isfinite(l2) && l2 > 0.0f) ? 1.0f / std::sqrt(l2) : 0.0f;
    for (int k = 0; k < 3; k++) F.sun[k] = (std::isfinite(l2) && l2 > 0.0f) ? L[k] * inv : 0.0f;
    const float g = pass->anisotropy, g2 = g * g;
    F.one_plus_g2 = 1.0f + g2;
    F.minus_2g = -2.0f * g;
    F.one_minus_g2 = 1.0f - g2;
  }
  F.shadow = shadow;
  F.edge = pass->edge_sharpness;
  F.frame = pass->frame_index;
  F.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(op));
}

// ---------------------------------------------------------------- the depth of field pass (include/svr_dof.h)
static_assert(sizeof(SvrDofPass) == 20 && offsetof(SvrDofPass, inv_z_scale) == 0 && offsetof(SvrDofPass, inv_z_bias) == 4 &&
                  offsetof(SvrDofPass, focus_distance) == 8 && offsetof(SvrDofPass, blur_scale) == 12 && offsetof(SvrDofPass, max_radius) == 16,
              "include/svr_dof.h");

int svr_dof_pass(SvrContext* ctx, const SvrDofPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_dof_pass: null argument");
  if (!(std::isfinite(pass->inv_z_scale) && std::isfinite(pass->inv_z_bias))) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_dof_pass: inv_z_scale and inv_z_bias must be finite");
  if (!(std::isfinite(pass->focus_distance) && pass->focus_distance > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_dof_pass: the focus distance must be finite and greater than 0");
  if (!(std::isfinite(pass->blur_scale) && pass->blur_scale >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_dof_pass: the blur scale must be finite and at least 0");
  if (!(pass->max_radius >= 0.0f && pass->max_radius <= (float)SVR_DOF_MAX_RADIUS))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_dof_pass: max_radius must be in 0..SVR_DOF_MAX_RADIUS");
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_dof_pass: the colour target must be RGBA16F (the pass works in scene-linear HDR)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_dof_pass: not under svr_set_row_interleave with a stride above 1");
  if (pass->blur_scale == 0.0f || pass->max_radius == 0.0f) return SVR_OK;  // a pinhole: the target keeps its bits, and no kernel is enqueued to rewrite them
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  // (both counts grow with the image's extent, so the images of any scissor fit in those of the whole target)
  const size_t texels = dof_texels(ctx->W, ctx->H);
  if (!ctx->d_dof) DEV_ALLOC(ctx->d_dof, texels * sizeof(uint2) + dof_cells(ctx->W, ctx->H) * sizeof(float));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  DofOp op;
  DofLaunch& D = op.launch;
  D.color = (uint2*)ctx->color;
  D.depth = ctx->depth;
  D.W = ctx->W;
  D.sx = ctx->sx;
  D.sy = ctx->sy;
  D.sw = ctx->sw;
  D.sh = ctx->sh;
  D.pitch = (ctx->sw + 1u) & ~1u;
  D.cw = (ctx->sw + 7u) / 8u;
  D.ch = (ctx->sh + 7u) / 8u;
  D.prep = ctx->d_dof.get();
  D.cells = reinterpret_cast<float*>(ctx->d_dof.get() + texels);
  D.inv_z_scale = pass->inv_z_scale;
  D.inv_z_bias = pass->inv_z_bias;
  D.neg_focus = -pass->focus_distance;
  D.blur_scale = pass->blur_scale;
  D.max_radius = pass->max_radius;
  D.neg_max_radius = -pass->max_radius;
  D.Rc = ((uint32_t)std::ceil(pass->max_radius) + 7u) / 8u;  // C63: R = 1 .. SVR_DOF_MAX_RADIUS, Rc = 1 or 2
  D.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(op));
}

// ---------------------------------------------------------------- the motion blur pass (include/svr_motion.h)
static_assert(sizeof(SvrMotionBlurPass) == 72 && offsetof(SvrMotionBlurPass, reproject) == 0 && offsetof(SvrMotionBlurPass, shutter) == 64 &&
                  offsetof(SvrMotionBlurPass, max_blur) == 68,
              "include/svr_motion.h");

int svr_motion_blur_pass(SvrContext* ctx, const SvrMotionBlurPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_motion_blur_pass: null argument");
  if (int e = finite_matrix("svr_motion_blur_pass", "reproject", pass->reproject)) return e;
  if (!(std::isfinite(pass->shutter) && pass->shutter >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_motion_blur_pass: the shutter must be finite and at least 0");
  if (!(pass->max_blur >= 0.0f && pass->max_blur <= (float)SVR_MOTION_MAX_BLUR))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_motion_blur_pass: max_blur must be in 0..SVR_MOTION_MAX_BLUR");
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_motion_blur_pass: the colour target must be RGBA16F (the pass works in scene-linear HDR)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_motion_blur_pass: not under svr_set_row_interleave with a stride above 1");
  if (pass->shutter == 0.0f || pass->max_blur == 0.0f) return SVR_OK;  // a closed shutter: the target keeps its bits, and no kernel is enqueued to rewrite them
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  // (both counts grow with the image's extent, so the images of any scissor fit in those of the whole target)
  const size_t texels = motion_texels(ctx->W, ctx->H);
  if (!ctx->d_motion) DEV_ALLOC(ctx->d_motion, texels * sizeof(uint4) + motion_cells(ctx->W, ctx->H) * sizeof(unsigned long long));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  MotionOp op;
  MotionLaunch& M = op.launch;
  M.color = (uint2*)ctx->color;
  M.depth = ctx->depth;
  M.W = ctx->W;
  M.sx = ctx->sx;
  M.sy = ctx->sy;
  M.sw = ctx->sw;
  M.sh = ctx->sh;
  M.cw = (ctx->sw + 7u) / 8u;
  M.ch = (ctx->sh + 7u) / 8u;
  M.prep = ctx->d_motion.get();
  M.cells = reinterpret_cast<unsigned long long*>(ctx->d_motion.get() + texels);
  std::memcpy(M.reproject, pass->reproject, sizeof(M.reproject));
  M.two_over_w = 2.0f / (float)ctx->W;
  M.two_over_h = 2.0f / (float)ctx->H;
  M.half_w = (float)ctx->W * 0.5f;
  M.half_h = (float)ctx->H * 0.5f;
  M.half_shutter = 0.5f * pass->shutter;
  M.max_blur = pass->max_blur;
  M.Rc = ((uint32_t)std::ceil(pass->max_blur) + 7u) / 8u;  // C69: R = 1 .. SVR_MOTION_MAX_BLUR, Rc = 1 or 2
  M.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(op));
}

// ---------------------------------------------------------------- the reflection pass (include/svr_reflect.h)
static_assert(sizeof(SvrReflectPass) == 192 && offsetof(SvrReflectPass, inv_viewproj) == 64 && offsetof(SvrReflectPass, camera_position) == 128 &&
                  offsetof(SvrReflectPass, inv_z_scale) == 140 && offsetof(SvrReflectPass, steps) == 152 && offsetof(SvrReflectPass, thickness) == 160 &&
                  offsetof(SvrReflectPass, resolve) == 180 && offsetof(SvrReflectPass, frame_index) == 188,
              "include/svr_reflect.h");

int svr_reflect_pass(SvrContext* ctx, const SvrReflectPass* pass) {
  const std::string who = "svr_reflect_pass: ";
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, who + "null argument");
  if (int e = finite_matrix("svr_reflect_pass", "viewproj", pass->viewproj)) return e;
  if (int e = finite_matrix("svr_reflect_pass", "inv_viewproj", pass->inv_viewproj)) return e;
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(pass->camera_position[k])) return fail(SVR_ERR_INVALID_ARGUMENT, who + "camera_position must be finite");
  if (!(std::isfinite(pass->inv_z_scale) && std::isfinite(pass->inv_z_bias))) return fail(SVR_ERR_INVALID_ARGUMENT, who + "inv_z_scale and inv_z_bias must be finite");
  if (!(std::isfinite(pass->max_distance) && pass->max_distance > 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "max_distance must be finite and greater than 0");
  if (pass->steps < 1u || pass->steps > SVR_REFLECT_MAX_STEPS) return fail(SVR_ERR_INVALID_ARGUMENT, who + "steps must be in 1..SVR_REFLECT_MAX_STEPS");
  if (pass->refine > SVR_REFLECT_MAX_REFINE) return fail(SVR_ERR_INVALID_ARGUMENT, who + "refine must be in 0..SVR_REFLECT_MAX_REFINE");
  if (!(std::isfinite(pass->thickness) && pass->thickness >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "the thickness must be finite and at least 0");
  if (!(pass->f0 >= 0.0f && pass->f0 <= 1.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "f0 must be in 0..1");
  if (!(std::isfinite(pass->intensity) && pass->intensity >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "the intensity must be finite and at least 0");
  if (!(pass->distance_fade >= 0.0f && pass->distance_fade <= 1.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "distance_fade must be in 0..1");
  if (!(std::isfinite(pass->edge_width) && pass->edge_width >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "the edge width must be finite and at least 0");
  if (pass->resolve > 1u) return fail(SVR_ERR_INVALID_ARGUMENT, who + "resolve must be 0 or 1");
  if (!(std::isfinite(pass->depth_tolerance) && pass->depth_tolerance >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, who + "the depth tolerance must be finite and at least 0");
  if (!ctx->attr[2] || !ctx->attr[3])
    return fail(SVR_ERR_INVALID_ARGUMENT, who + "needs the SVR_ATTR_NORMAL and SVR_ATTR_ALBEDO planes (svr_enable_attributes / svr_bind_attribute_target)");
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, who + "the colour target must be RGBA16F (the pass works in scene-linear HDR)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, who + "not under svr_set_row_interleave with a stride above 1");
  if (pass->intensity == 0.0f) return SVR_OK;  // no reflection: the target keeps its bits, and no kernel is enqueued to rewrite them
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  // (both counts grow with the image's extent, so the images of any scissor fit in those of the whole target)
  const size_t texels = reflect_texels(ctx->W, ctx->H);
  if (!ctx->d_reflect) DEV_ALLOC(ctx->d_reflect, texels * sizeof(float4) + reflect_cells(ctx->W, ctx->H) * sizeof(uint32_t));
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  ReflectOp op;
  ReflectLaunch& R = op.launch;
  R.color = (uint2*)ctx->color;
  R.depth = ctx->depth;
  R.normal = (const float4*)ctx->attr[2];
  R.albedo = (const float4*)ctx->attr[3];
  R.W = ctx->W;
  R.sx = ctx->sx;
  R.sy = ctx->sy;
  R.sw = ctx->sw;
  R.sh = ctx->sh;
  R.cw = (ctx->sw + 7u) / 8u;
  R.ch = (ctx->sh + 7u) / 8u;
  R.trace = ctx->d_reflect.get();
  R.cells = reinterpret_cast<uint32_t*>(ctx->d_reflect.get() + texels);
  R.two_over_w = 2.0f / (float)ctx->W;
  R.two_over_h = 2.0f / (float)ctx->H;
  R.half_w = (float)ctx->W * 0.5f;
  R.half_h = (float)ctx->H * 0.5f;
  R.x_lo = (float)ctx->sx;
  R.x_hi = (float)(ctx->sx + ctx->sw);
  R.y_lo = (float)ctx->sy;
  R.y_hi = (float)(ctx->sy + ctx->sh);
  std::memcpy(R.viewproj, pass->viewproj, sizeof(R.viewproj));
  std::memcpy(R.inv_viewproj, pass->inv_viewproj, sizeof(R.inv_viewproj));
  std::memcpy(R.cam, pass->camera_position, sizeof(R.cam));
  R.inv_z_scale = pass->inv_z_scale;
  R.inv_z_bias = pass->inv_z_bias;
  R.delta = pass->max_distance / (float)pass->steps;  // C75
  R.rmax = 1.0f / pass->max_distance;                 // C77
  R.steps = pass->steps;
  R.refine = pass->refine;
  R.q_max = 1.0f + pass->thickness;
  R.f0 = pass->f0;
  R.one_minus_f0 = 1.0f - pass->f0;
  R.intensity = pass->intensity;
  R.distance_fade = pass->distance_fade;
  R.inv_edge = pass->edge_width > 0.0f ? 1.0f / pass->edge_width : 0.0f;
  R.resolve = pass->resolve;
  R.depth_tolerance = pass->depth_tolerance;
  R.frame = pass->frame_index;
  R.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(op));
}

// ---------------------------------------------------------------- auto-exposure (include/svr_exposure.h)
static_assert(sizeof(SvrExposureMeter) == 24 && sizeof(SvrExposureState) == 24 && offsetof(SvrExposureState, exposure) == 0, "include/svr_exposure.h");
static_assert(sizeof(SvrExposureState) <= EXPOSURE_STATE_WORDS * sizeof(uint32_t), "the state's words");

// the state, the working bins and the last histogram: allocated and initialised by the first call that needs them
static int exposure_memory(SvrContext* ctx) {
  if (ctx->d_exposure) return SVR_OK;
  static const SvrExposureState first = {1.0f, 1.0f, 0.0f, 0u, 0u, 0u};
  if (int e = use_device(ctx)) return e;
  DevPtr<uint32_t> mem;
  DEV_ALLOC(mem, EXPOSURE_WORDS * sizeof(uint32_t));
  HIPCHK(hipMemsetAsync(mem.get(), 0, EXPOSURE_WORDS * sizeof(uint32_t), ctx->stream));
  HIPCHK(hipMemcpyAsync(mem.get(), &first, sizeof(first), hipMemcpyHostToDevice, ctx->stream));
  ctx->d_exposure = std::move(mem);
  return SVR_OK;
}

int svr_meter_exposure(SvrContext* ctx, const SvrExposureMeter* meter) {
  if (!ctx || !meter) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: null argument");
  if (!(std::isfinite(meter->key) && meter->key > 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: the key must be finite and greater than 0");
  if (!(meter->low_fraction >= 0.0f && meter->low_fraction < 1.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: low_fraction must be at least 0 and less than 1");
  if (!(meter->high_fraction > meter->low_fraction && meter->high_fraction <= 1.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: high_fraction must be greater than low_fraction and at most 1");
  if (!(std::isfinite(meter->min_exposure) && meter->min_exposure > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: min_exposure must be finite and greater than 0");
  if (!(std::isfinite(meter->max_exposure) && meter->max_exposure >= meter->min_exposure))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: max_exposure must be finite and at least min_exposure");
  if (!(meter->adapt >= 0.0f && meter->adapt <= 1.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_meter_exposure: adapt must be at least 0 and at most 1");
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_meter_exposure: the colour target must be RGBA16F");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_meter_exposure: not under svr_set_row_interleave with a stride above 1");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  if (int e = exposure_memory(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;  // this call reads colour: a deferred clear lands first
  ExposureOp E{};
  E.color = (const uint2*)ctx->color;
  E.W = ctx->W;
  E.sx = ctx->sx;
  E.sy = ctx->sy;
  E.sw = ctx->sw;
  E.sh = ctx->sh;
  E.mem = ctx->d_exposure.get();
  E.meter = *meter;
  // decided here, in call order, and it travels with the operation: a replay finds it as it was
  E.snap = ctx->exposure_snap ? 1u : 0u;
  E.poison = ctx->d_poison.get();
  if (int e = log_op(ctx, std::move(E))) return e;
  ctx->exposure_snap = false;
  return SVR_OK;
}

int svr_reset_exposure(SvrContext* ctx) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_reset_exposure: null context");
  ctx->exposure_snap = true;
  return SVR_OK;
}

int svr_set_post_auto_exposure(SvrContext* ctx, int on) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_set_post_auto_exposure: null context");
  ctx->post_auto = on != 0;
  return SVR_OK;
}

int svr_read_exposure(SvrContext* ctx, SvrExposureState* out) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_exposure: null argument");
  if (int e = exposure_memory(ctx)) return e;
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(out, ctx->d_exposure.get(), sizeof(SvrExposureState), hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_debug_read_exposure_histogram(SvrContext* ctx, uint32_t* out, size_t bytes) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_exposure_histogram: null argument");
  if (bytes != SVR_EXPOSURE_BINS * sizeof(uint32_t)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_exposure_histogram: the size is not SVR_EXPOSURE_BINS * 4");
  if (int e = exposure_memory(ctx)) return e;
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(out, ctx->d_exposure.get() + EXPOSURE_STATE_WORDS + EXPOSURE_BINS_WORDS, bytes, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_get_exposure_state(SvrContext* ctx, const void** device) {
  if (!ctx || !device) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_exposure_state: null argument");
  if (int e = exposure_memory(ctx)) return e;
  *device = ctx->d_exposure.get();
  return SVR_OK;
}

// ---------------------------------------------------------------- temporal antialiasing (include/svr_temporal.h)
static bool temporal_history_usable(const SvrContext* ctx) {
  return ctx->temporal_has && ctx->temporal_scissor[0] == ctx->sx && ctx->temporal_scissor[1] == ctx->sy &&
         ctx->temporal_scissor[2] == ctx->sw && ctx->temporal_scissor[3] == ctx->sh;
}

int svr_temporal_resolve(SvrContext* ctx, const SvrTemporalPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_temporal_resolve: null argument");
  if (!(std::isfinite(pass->blend) && pass->blend > 0.0f && pass->blend <= 1.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_temporal_resolve: the blend must be finite, greater than 0 and at most 1");
  if (pass->flags & ~(uint32_t)(SVR_TEMPORAL_RESET | SVR_TEMPORAL_NO_CLAMP)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_temporal_resolve: unknown flag bits");
  if (int e = finite_matrix("svr_temporal_resolve", "reproject", pass->reproject)) return e;
  if (ctx->fmt != SVR_COLOR_RGBA16F) return fail(SVR_ERR_UNSUPPORTED, "svr_temporal_resolve: the colour target must be RGBA16F");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_temporal_resolve: not under svr_set_row_interleave with a stride above 1");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  const size_t hist_bytes = (size_t)ctx->W * ctx->H * sizeof(uint2);
  for (int i = 0; i < 2; i++)
    if (!ctx->d_temporal[i]) {  // zeroed once: the read-back hook shows the whole extent, the kernels read the scissor only
      DEV_ALLOC(ctx->d_temporal[i], hist_bytes);
      HIPCHK(hipMemsetAsync(ctx->d_temporal[i].get(), 0, hist_bytes, ctx->stream));
    }
  if (int e = flush_clear(ctx)) return e;  // this call writes colour: a deferred clear lands first
  TemporalOp T{};
  T.color = (uint2*)ctx->color;
  T.depth = ctx->depth;
  T.W = ctx->W;
  T.H = ctx->H;
  T.sx = ctx->sx;
  T.sy = ctx->sy;
  T.sw = ctx->sw;
  T.sh = ctx->sh;
  // the roles and the validity are decided here, in call order, and travel with the operation: a replay finds them as they were
  T.hist_in = ctx->d_temporal[ctx->temporal_read].get();
  T.hist_out = ctx->d_temporal[ctx->temporal_read ^ 1].get();
  T.history_valid = temporal_history_usable(ctx) && !(pass->flags & SVR_TEMPORAL_RESET) ? 1u : 0u;
  T.clamp = (pass->flags & SVR_TEMPORAL_NO_CLAMP) ? 0u : 1u;
  std::memcpy(T.reproject, pass->reproject, sizeof(T.reproject));
  T.blend = pass->blend;
  T.two_over_w = 2.0f / (float)ctx->W;
  T.two_over_h = 2.0f / (float)ctx->H;
  T.half_w = (float)ctx->W * 0.5f;
  T.half_h = (float)ctx->H * 0.5f;
  T.poison = ctx->d_poison.get();
  if (int e = log_op(ctx, std::move(T))) return e;
  ctx->temporal_read ^= 1;
  ctx->temporal_has = true;
  ctx->temporal_scissor[0] = ctx->sx;
  ctx->temporal_scissor[1] = ctx->sy;
  ctx->temporal_scissor[2] = ctx->sw;
  ctx->temporal_scissor[3] = ctx->sh;
  return SVR_OK;
}

int svr_debug_read_temporal_history(SvrContext* ctx, void* dst, size_t bytes, uint32_t* valid) {
  if (!ctx || !valid) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_temporal_history: null argument");
  const size_t need = (size_t)ctx->W * ctx->H * sizeof(uint2);
  if (dst && bytes < need) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_temporal_history: buffer too small");
  if (int e = svr_sync(ctx)) return e;
  *valid = temporal_history_usable(ctx) ? 1u : 0u;
  if (!dst) return SVR_OK;
  if (ctx->d_temporal[ctx->temporal_read])
    HIPCHK(hipMemcpy(dst, ctx->d_temporal[ctx->temporal_read].get(), need, hipMemcpyDeviceToHost));
  else
    std::memset(dst, 0, need);
  return SVR_OK;
}

// ---------------------------------------------------------------- ambient occlusion (include/svr_ambient.h)
static float* ambient_target(const SvrContext* ctx) { return ctx->ambient_bound ? ctx->ambient_bound : ctx->d_ambient_own.get(); }

int svr_ambient_pass(SvrContext* ctx, const SvrAmbientPass* pass) {
  if (!ctx || !pass) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: null argument");
  if (!(std::isfinite(pass->radius) && pass->radius > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: the radius must be finite and greater than 0");
  if (!(std::isfinite(pass->pixels_per_unit) && pass->pixels_per_unit > 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: pixels_per_unit must be finite and greater than 0");
  if (!(std::isfinite(pass->bias) && pass->bias >= 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: the bias must be finite and at least 0");
  if (!(std::isfinite(pass->intensity) && pass->intensity >= 0.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: the intensity must be finite and at least 0");
  if (!(std::isfinite(pass->sharpness) && pass->sharpness >= 0.0f && pass->sharpness < 1.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: the sharpness must be finite, at least 0 and less than 1");
  if (pass->flags & ~(uint32_t)SVR_AMBIENT_NO_BLUR) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: unknown flag bits");
  if (int e = finite_matrix("svr_ambient_pass", "inv_viewproj", pass->inv_viewproj)) return e;
  if (!ctx->attr[2]) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_ambient_pass: needs the SVR_ATTR_NORMAL plane (svr_enable_attributes / svr_bind_attribute_target)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, "svr_ambient_pass: not under svr_set_row_interleave with a stride above 1");
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  const size_t n = (size_t)ctx->W * ctx->H;
  // zeroed once: the read-backs show the whole extent, the kernels touch the scissor only
  if (!ctx->d_ambient_raw) {
    DEV_ALLOC(ctx->d_ambient_raw, n * sizeof(float2));
    HIPCHK(hipMemsetAsync(ctx->d_ambient_raw.get(), 0, n * sizeof(float2), ctx->stream));
  }
  if (!ctx->ambient_bound && !ctx->d_ambient_own) {
    DEV_ALLOC(ctx->d_ambient_own, n * sizeof(float));
    HIPCHK(hipMemsetAsync(ctx->d_ambient_own.get(), 0, n * sizeof(float), ctx->stream));
  }
  // (no flush_clear: the pass neither reads nor writes colour)
  AmbientOp T{};
  T.depth = ctx->depth;
  T.normal = (const float4*)ctx->attr[2];
  T.raw = ctx->d_ambient_raw.get();
  T.out = ambient_target(ctx);
  T.W = ctx->W;
  T.H = ctx->H;
  T.sx = ctx->sx;
  T.sy = ctx->sy;
  T.sw = ctx->sw;
  T.sh = ctx->sh;
  std::memcpy(T.inv_viewproj, pass->inv_viewproj, sizeof(T.inv_viewproj));
  T.two_over_w = 2.0f / (float)ctx->W;
  T.two_over_h = 2.0f / (float)ctx->H;
  T.radius_px = pass->radius * pass->pixels_per_unit;
  T.radius2 = pass->radius * pass->radius;
  T.bias = pass->bias;
  T.coef = (pass->intensity * pass->radius) * 0.125f;
  T.sharpness = pass->sharpness;
  T.blur = (pass->flags & SVR_AMBIENT_NO_BLUR) ? 0u : 1u;
  T.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(T));
}

int svr_bind_ambient_target(SvrContext* ctx, float* dev) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  if (((uintptr_t)dev & 15u) != 0u) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_bind_ambient_target: the target must be 16-byte aligned");
  if (int e = use_device(ctx)) return e;
  // no fence: passes already enqueued carry their own planes (also for a replay), as with svr_bind_attribute_target
  if (int e = poll_pending(ctx)) return e;
  ctx->ambient_bound = dev;
  return SVR_OK;
}

int svr_get_ambient_target(SvrContext* ctx, float** dev) {
  if (!ctx || !dev) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_get_ambient_target: null argument");
  *dev = ambient_target(ctx);
  return SVR_OK;
}

int svr_read_ambient(SvrContext* ctx, void* dst_host, size_t bytes) {
  if (!ctx || !dst_host) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ambient: null argument");
  if (!ambient_target(ctx)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ambient: no ambient target (svr_ambient_pass / svr_bind_ambient_target)");
  if (bytes != (size_t)ctx->W * ctx->H * sizeof(float)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_ambient: the size is not the plane's");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(dst_host, ambient_target(ctx), bytes, hipMemcpyDeviceToHost));
  return SVR_OK;
}

int svr_set_light_ambient_occlusion(SvrContext* ctx, int on) {
  if (!ctx) return fail(SVR_ERR_INVALID_ARGUMENT, "null context");
  ctx->light_ao = on != 0;
  return SVR_OK;
}

int svr_debug_read_ambient_raw(SvrContext* ctx, void* dst_host, size_t bytes) {
  if (!ctx || !dst_host) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_ambient_raw: null argument");
  if (!ctx->d_ambient_raw) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_ambient_raw: no ambient pass yet");
  if (bytes != (size_t)ctx->W * ctx->H * sizeof(float2)) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_ambient_raw: the size is not the plane's");
  if (int e = svr_sync(ctx)) return e;
  HIPCHK(hipMemcpy(dst_host, ctx->d_ambient_raw.get(), bytes, hipMemcpyDeviceToHost));
  return SVR_OK;
}

// ---------------------------------------------------------------- the UI overlay pass (include/svr_overlay.h)
static_assert(sizeof(SvrOverlayVertex) == 20 && sizeof(SvrOverlayCmd) == 32 && sizeof(SvrOverlayTexture) == 24 && sizeof(SvrOverlayStats) == 12,
              "include/svr_overlay.h");

int svr_draw_overlay(SvrContext* ctx, void* dst_dev, uint32_t dw, uint32_t dh, int fmt, const SvrOverlayList* list) {
  const std::string who = "svr_draw_overlay: ";
  if (!ctx || !dst_dev || !list) return fail(SVR_ERR_INVALID_ARGUMENT, who + "null argument");
  if (dw == 0 || dh == 0 || dw > 16384 || dh > 16384) return fail(SVR_ERR_INVALID_ARGUMENT, who + "extent must be in 1..16384");
  if (fmt != SVR_SWAPCHAIN_B8G8R8A8 && fmt != SVR_SWAPCHAIN_R8G8B8A8) return fail(SVR_ERR_INVALID_ARGUMENT, who + "unknown format");
  if (list->n_cmds > SVR_OVERLAY_MAX_CMDS) return fail(SVR_ERR_INVALID_ARGUMENT, who + "n_cmds is above SVR_OVERLAY_MAX_CMDS");
  if (list->n_textures > SVR_OVERLAY_MAX_TEXTURES) return fail(SVR_ERR_INVALID_ARGUMENT, who + "n_textures is above SVR_OVERLAY_MAX_TEXTURES");
  if ((list->n_cmds && !list->cmds) || (list->n_vertices && !list->vertices) || (list->n_indices && !list->indices) || (list->n_textures && !list->textures))
    return fail(SVR_ERR_INVALID_ARGUMENT, who + "null array with a count above 0");
  for (int k = 0; k < 2; k++) {
    if (!std::isfinite(list->display_pos[k])) return fail(SVR_ERR_INVALID_ARGUMENT, who + "display_pos must be finite");
    if (!(std::isfinite(list->scale[k]) && list->scale[k] > 0.0f)) return fail(SVR_ERR_INVALID_ARGUMENT, who + "scale must be finite and greater than 0");
  }
  for (uint32_t i = 0; i < list->n_textures; i++) {
    const SvrOverlayTexture& t = list->textures[i];
    const std::string which = "texture " + std::to_string(i);
    if (!t.texels) return fail(SVR_ERR_INVALID_ARGUMENT, who + which + " has a null pointer");
    if (t.width == 0 || t.height == 0 || t.width > SVR_OVERLAY_MAX_TEXTURE_EXTENT || t.height > SVR_OVERLAY_MAX_TEXTURE_EXTENT)
      return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": extent must be in 1..16384");
    if (t.format != SVR_OVERLAY_TEX_RGBA8 && t.format != SVR_OVERLAY_TEX_A8) return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": unknown format");
  }
  uint64_t submitted = 0;
  for (uint32_t c = 0; c < list->n_cmds; c++) {
    const SvrOverlayCmd& cmd = list->cmds[c];
    const std::string which = "command " + std::to_string(c);
    if (cmd.elem_count % 3u) return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": elem_count is not divisible by 3");
    if ((uint64_t)cmd.idx_offset + cmd.elem_count > list->n_indices) return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": idx_offset + elem_count is above n_indices");
    if (cmd.elem_count == 0) continue;
    if (cmd.texture >= list->n_textures) return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": texture is not below n_textures");
    for (uint32_t i = 0; i < cmd.elem_count; i++)
      if ((uint64_t)cmd.vtx_offset + list->indices[cmd.idx_offset + i] >= list->n_vertices)
        return fail(SVR_ERR_INVALID_ARGUMENT, who + which + ": index out of range (vtx_offset + index >= n_vertices)");
    submitted += cmd.elem_count / 3u;
    if (submitted > SVR_OVERLAY_MAX_TRIANGLES) return fail(SVR_ERR_INVALID_ARGUMENT, who + "more than SVR_OVERLAY_MAX_TRIANGLES triangles");
  }
  // C45: the clip boxes, in whole pixels; a command without triangles or with an empty box does not reach the device
  OverlayOp op;
  uint32_t n_tris = 0, vtx_end = 0, idx_end = 0;
  int32_t reach[4] = {(int32_t)dw, (int32_t)dh, 0, 0};  // the union of the live commands' clip boxes
  const float ext[2] = {(float)dw, (float)dh};
  for (uint32_t c = 0; c < list->n_cmds; c++) {
    const SvrOverlayCmd& cmd = list->cmds[c];
    if (cmd.elem_count == 0) continue;
    int32_t lo[2];
    uint32_t span[2];
    bool empty = false;
    for (int k = 0; k < 2; k++) {
      float cmin = (cmd.clip_rect[k] - list->display_pos[k]) * list->scale[k], cmax = (cmd.clip_rect[2 + k] - list->display_pos[k]) * list->scale[k];
      if (cmin < 0.0f) cmin = 0.0f;
      if (cmax > ext[k]) cmax = ext[k];
      if (!(cmax > cmin)) {  // also where one of them is NaN
        empty = true;
        break;
      }
      lo[k] = (int32_t)cmin;
      span[k] = (uint32_t)(cmax - cmin);
    }
    if (empty) continue;
    OverlayCmdDev d{};
    d.x0 = lo[0];
    d.y0 = lo[1];
    d.x1 = std::min<int32_t>(lo[0] + (int32_t)span[0], (int32_t)dw);  // (the min never binds: DESIGN.md C45)
    d.y1 = std::min<int32_t>(lo[1] + (int32_t)span[1], (int32_t)dh);
    if (d.x1 <= d.x0 || d.y1 <= d.y0) continue;  // a box narrower than a pixel passes none
    d.texture = cmd.texture;
    d.vtx_offset = cmd.vtx_offset;
    d.idx_offset = cmd.idx_offset;
    d.tri_first = n_tris;
    d.tri_count = cmd.elem_count / 3u;
    n_tris += d.tri_count;
    idx_end = std::max(idx_end, cmd.idx_offset + cmd.elem_count);
    for (uint32_t i = 0; i < cmd.elem_count; i++) vtx_end = std::max(vtx_end, cmd.vtx_offset + list->indices[cmd.idx_offset + i] + 1u);
    reach[0] = std::min(reach[0], d.x0);
    reach[1] = std::min(reach[1], d.y0);
    reach[2] = std::max(reach[2], d.x1);
    reach[3] = std::max(reach[3], d.y1);
    op.cmds.push_back(d);
  }
  if (n_tris == 0) return SVR_OK;  // nothing to draw: nothing is enqueued
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  // (the colour target is not touched: a deferred svr_clear_color stays deferred)
  op.submitted = (uint32_t)submitted;
  op.vertices.assign(list->vertices, list->vertices + vtx_end);  // what the live commands can name
  op.indices.assign(list->indices, list->indices + idx_end);
  op.textures.assign(list->textures, list->textures + list->n_textures);
  OverlayLaunch& L = op.launch;
  L.dst = static_cast<uint32_t*>(dst_dev);
  L.dw = dw;
  L.dh = dh;
  L.dst_fmt = fmt;
  for (int k = 0; k < 2; k++) {
    L.display_pos[k] = list->display_pos[k];
    L.scale[k] = list->scale[k];
  }
  L.n_cmds = (uint32_t)op.cmds.size();
  L.n_tris = n_tris;
  L.n_textures = list->n_textures;
  // no tile outside every clip box has work: they are not launched (0 <= x0 < x1 <= dw for every live command)
  L.tile_x0 = (uint32_t)reach[0] / 32u;
  L.tile_y0 = (uint32_t)reach[1] / 32u;
  L.tiles_w = ((uint32_t)reach[2] + 31u) / 32u - L.tile_x0;
  L.tiles_h = ((uint32_t)reach[3] + 31u) / 32u - L.tile_y0;
  L.poison = ctx->d_poison.get();
  return log_op(ctx, std::move(op));
}

int svr_debug_read_overlay_stats(SvrContext* ctx, SvrOverlayStats* out) {
  if (!ctx || !out) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_debug_read_overlay_stats: null argument");
  if (int e = svr_sync(ctx)) return e;
  SvrOverlayStats st = {0u, 0u, 0u};
  if (ctx->d_overlay_in.p) HIPCHK(hipMemcpy(&st, ctx->d_overlay_in.p, sizeof(st), hipMemcpyDeviceToHost));
  *out = st;
  return SVR_OK;
}

int svr_overlay_font(const uint8_t** a8, uint32_t* width, uint32_t* height, uint32_t* cell_w, uint32_t* cell_h, uint32_t* first_char, uint32_t* n_chars) {
  static const std::vector<uint8_t> atlas = build_font_atlas();
  static_assert(SVR_OVERLAY_FONT_WHITE_X == FONT_W - FONT_CELL_W + 2 && SVR_OVERLAY_FONT_WHITE_Y == FONT_H - FONT_CELL_H + 3, "the opaque texel lies inside the filled cell");
  if (a8) *a8 = atlas.data();
  if (width) *width = FONT_W;
  if (height) *height = FONT_H;
  if (cell_w) *cell_w = FONT_CELL_W;
  if (cell_h) *cell_h = FONT_CELL_H;
  if (first_char) *first_char = FONT_FIRST;
  if (n_chars) *n_chars = FONT_CHARS;
  return SVR_OK;
}

// ---------------------------------------------------------------- the upscaled present (include/svr_upscale.h)
static_assert(sizeof(SvrUpscalePass) == 8, "include/svr_upscale.h");

// the checks of both entry points, then the kernel's parameters; nothing of the context changes
static int upscale_launch(SvrContext* ctx, const SvrUpscalePass* pass, void* dst, uint32_t dw, uint32_t dh, int fmt, const char* who, UpscaleLaunch* out) {
  const std::string fn(who);
  if (!pass) return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": null argument");
  if (int e = blit_checks(ctx, dst, dw, dh, fmt, who)) return e;
  if (!(std::isfinite(pass->sharpness) && pass->sharpness >= 0.0f && pass->sharpness <= 1.0f))
    return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": the sharpness must be finite, at least 0 and at most 1");
  if (pass->flags & ~(uint32_t)SVR_UPSCALE_NO_SHARPEN) return fail(SVR_ERR_INVALID_ARGUMENT, fn + ": unknown flag bits");
  if (dw < ctx->W || dh < ctx->H) return fail(SVR_ERR_UNSUPPORTED, fn + ": the destination is smaller than the colour target (svr_copy_to_swapchain minifies)");
  if (ctx->rstride > 1u) return fail(SVR_ERR_UNSUPPORTED, fn + ": not under svr_set_row_interleave with a stride above 1");
  UpscaleLaunch& U = *out;
  U = UpscaleLaunch{};
  U.src = ctx->color;
  U.src_fmt = ctx->fmt;
  U.W = ctx->W;
  U.H = ctx->H;
  U.dst = static_cast<uint32_t*>(dst);
  U.dw = dw;
  U.dh = dh;
  U.dst_fmt = fmt;
  U.su = (float)ctx->W / (float)dw;  // C51
  U.sv = (float)ctx->H / (float)dh;
  U.peak = -1.0f / (8.0f - 3.0f * pass->sharpness);  // C53: computed once, here; it travels in the operation by value
  U.sharpen = (pass->flags & SVR_UPSCALE_NO_SHARPEN) ? 0u : 1u;
  U.poison = ctx->d_poison.get();
  return SVR_OK;
}

int svr_upscale_to_swapchain(SvrContext* ctx, const SvrUpscalePass* pass, void* dst_dev, uint32_t dw, uint32_t dh, int fmt) {
  UpscaleOp op;
  if (int e = upscale_launch(ctx, pass, dst_dev, dw, dh, fmt, "svr_upscale_to_swapchain", &op)) return e;
  if (int e = use_device(ctx)) return e;
  if (int e = poll_pending(ctx)) return e;
  if (int e = flush_clear(ctx)) return e;  // this call reads colour: a deferred clear lands first
  op.status = ctx->present_status;
  return log_op(ctx, std::move(op));
}

int svr_read_upscaled(SvrContext* ctx, const SvrUpscalePass* pass, uint32_t dw, uint32_t dh, int fmt, void* dst_host, size_t bytes) {
  UpscaleLaunch U;
  if (int e = upscale_launch(ctx, pass, dst_host, dw, dh, fmt, "svr_read_upscaled", &U)) return e;
  if (bytes < (size_t)dw * dh * 4) return fail(SVR_ERR_INVALID_ARGUMENT, "svr_read_upscaled: buffer too small");
  if (int e = use_device(ctx)) return e;
  if (int e = finish_pending(ctx)) return e;  // the read-back is a fence
  if (int e = ctx->d_cvt.ensure((size_t)dw * dh * 4)) return e;
  U.dst = static_cast<uint32_t*>(ctx->d_cvt.p);
  launch_upscale(U, 0u, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dst_host, ctx->d_cvt.p, (size_t)dw * dh * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return SVR_OK;
}

}  // extern "C"
