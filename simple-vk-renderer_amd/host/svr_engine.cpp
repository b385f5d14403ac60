// svr_engine.cpp — see svr_engine.h.  Every function names the reference code it stands for.
#include "svr_engine.h"
#include "svr_overlay_text.h"

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace svrhost {

bool SvrApi::load(const std::string& path, std::string* err) {
  handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!handle) {
    if (err) *err = dlerror();
    return false;
  }
  bool ok = true;
#define SVR_LOAD(name)                                                   \
  name = reinterpret_cast<decltype(name)>(dlsym(handle, #name));          \
  if (!name) {                                                           \
    ok = false;                                                          \
    if (err) *err = std::string("missing symbol ") + #name;              \
  }
  SVR_LOAD(svr_create) SVR_LOAD(svr_destroy) SVR_LOAD(svr_upload_mesh) SVR_LOAD(svr_create_image)
  SVR_LOAD(svr_create_sampler) SVR_LOAD(svr_write_material) SVR_LOAD(svr_clear_color) SVR_LOAD(svr_draw_geometry)
  SVR_LOAD(svr_sync) SVR_LOAD(svr_read_color) SVR_LOAD(svr_read_depth) SVR_LOAD(svr_get_stats) SVR_LOAD(svr_last_error)
  SVR_LOAD(svr_backend_name) SVR_LOAD(svr_draw_background) SVR_LOAD(svr_read_swapchain) SVR_LOAD(svr_copy_to_swapchain)
  SVR_LOAD(svr_set_option)
#undef SVR_LOAD
  // optional: only SvrEngine::retained needs them
  svr_create_draw_list = reinterpret_cast<decltype(svr_create_draw_list)>(dlsym(handle, "svr_create_draw_list"));
  svr_update_draw_list = reinterpret_cast<decltype(svr_update_draw_list)>(dlsym(handle, "svr_update_draw_list"));
  svr_destroy_draw_list = reinterpret_cast<decltype(svr_destroy_draw_list)>(dlsym(handle, "svr_destroy_draw_list"));
  svr_draw_list = reinterpret_cast<decltype(svr_draw_list)>(dlsym(handle, "svr_draw_list"));
  svr_enable_ids = reinterpret_cast<decltype(svr_enable_ids)>(dlsym(handle, "svr_enable_ids"));
  svr_pick = reinterpret_cast<decltype(svr_pick)>(dlsym(handle, "svr_pick"));
  svr_draw_geometry_views = reinterpret_cast<decltype(svr_draw_geometry_views)>(dlsym(handle, "svr_draw_geometry_views"));
  svr_draw_list_views = reinterpret_cast<decltype(svr_draw_list_views)>(dlsym(handle, "svr_draw_list_views"));
  svr_draw_depth = reinterpret_cast<decltype(svr_draw_depth)>(dlsym(handle, "svr_draw_depth"));
  svr_draw_list_depth = reinterpret_cast<decltype(svr_draw_list_depth)>(dlsym(handle, "svr_draw_list_depth"));
  svr_create_depth_pyramid = reinterpret_cast<decltype(svr_create_depth_pyramid)>(dlsym(handle, "svr_create_depth_pyramid"));
  svr_destroy_depth_pyramid = reinterpret_cast<decltype(svr_destroy_depth_pyramid)>(dlsym(handle, "svr_destroy_depth_pyramid"));
  svr_build_depth_pyramid = reinterpret_cast<decltype(svr_build_depth_pyramid)>(dlsym(handle, "svr_build_depth_pyramid"));
  svr_set_occlusion_pyramid = reinterpret_cast<decltype(svr_set_occlusion_pyramid)>(dlsym(handle, "svr_set_occlusion_pyramid"));
  svr_enable_attributes = reinterpret_cast<decltype(svr_enable_attributes)>(dlsym(handle, "svr_enable_attributes"));
  svr_light_pass = reinterpret_cast<decltype(svr_light_pass)>(dlsym(handle, "svr_light_pass"));
  svr_set_depth_load_op = reinterpret_cast<decltype(svr_set_depth_load_op)>(dlsym(handle, "svr_set_depth_load_op"));
  svr_post_pass = reinterpret_cast<decltype(svr_post_pass)>(dlsym(handle, "svr_post_pass"));
  svr_temporal_resolve = reinterpret_cast<decltype(svr_temporal_resolve)>(dlsym(handle, "svr_temporal_resolve"));
  svr_ambient_pass = reinterpret_cast<decltype(svr_ambient_pass)>(dlsym(handle, "svr_ambient_pass"));
  svr_set_light_ambient_occlusion = reinterpret_cast<decltype(svr_set_light_ambient_occlusion)>(dlsym(handle, "svr_set_light_ambient_occlusion"));
  svr_meter_exposure = reinterpret_cast<decltype(svr_meter_exposure)>(dlsym(handle, "svr_meter_exposure"));
  svr_set_post_auto_exposure = reinterpret_cast<decltype(svr_set_post_auto_exposure)>(dlsym(handle, "svr_set_post_auto_exposure"));
  svr_read_exposure = reinterpret_cast<decltype(svr_read_exposure)>(dlsym(handle, "svr_read_exposure"));
  svr_draw_overlay = reinterpret_cast<decltype(svr_draw_overlay)>(dlsym(handle, "svr_draw_overlay"));
  svr_overlay_font = reinterpret_cast<decltype(svr_overlay_font)>(dlsym(handle, "svr_overlay_font"));
  svr_upscale_to_swapchain = reinterpret_cast<decltype(svr_upscale_to_swapchain)>(dlsym(handle, "svr_upscale_to_swapchain"));
  svr_read_upscaled = reinterpret_cast<decltype(svr_read_upscaled)>(dlsym(handle, "svr_read_upscaled"));
  svr_fog_pass = reinterpret_cast<decltype(svr_fog_pass)>(dlsym(handle, "svr_fog_pass"));
  svr_dof_pass = reinterpret_cast<decltype(svr_dof_pass)>(dlsym(handle, "svr_dof_pass"));
  svr_motion_blur_pass = reinterpret_cast<decltype(svr_motion_blur_pass)>(dlsym(handle, "svr_motion_blur_pass"));
  svr_reflect_pass = reinterpret_cast<decltype(svr_reflect_pass)>(dlsym(handle, "svr_reflect_pass"));
  svr_read_attribute = reinterpret_cast<decltype(svr_read_attribute)>(dlsym(handle, "svr_read_attribute"));
  return ok;
}
void SvrApi::unload() {
  if (handle) dlclose(handle);
  handle = nullptr;
}

// ---------------------------------------------------------------- Camera (src/camera.cpp)
mat4 Camera::get_rotation_matrix() const {  // :61-66
  svrm::quat pitch_rotation = svrm::angle_axis(pitch, vec3{1, 0, 0});
  svrm::quat yaw_rotation = svrm::angle_axis(yaw, vec3{0, -1, 0});
  return svrm::mul(svrm::to_mat4(yaw_rotation), svrm::to_mat4(pitch_rotation));
}
mat4 Camera::get_view_matrix() const {  // :54-59
  mat4 camera_translation = svrm::translate(svrm::identity(), position);
  return svrm::inverse(svrm::mul(camera_translation, get_rotation_matrix()));
}
void Camera::update() {  // :8-11
  mat4 r = get_rotation_matrix();
  svrm::vec4 d = svrm::mul(r, svrm::vec4{velocity.x * 0.5f, velocity.y * 0.5f, velocity.z * 0.5f, 0.f});
  position.x += d.x;
  position.y += d.y;
  position.z += d.z;
}

// ---------------------------------------------------------------- scene graph
void Node::refresh_transform(const mat4& parent_matrix) {  // src/vk_types.h:157-163
  world_transform = svrm::mul(parent_matrix, local_transform);
  for (auto& c : children) c->refresh_transform(parent_matrix);  // NOT world_transform: the reference's quirk (D8)
}
void Node::Draw(const mat4& top_matrix, DrawContext& ctx) {  // src/vk_types.h:165-169
  for (auto& c : children) c->Draw(top_matrix, ctx);
}
void MeshNode::Draw(const mat4& top_matrix, DrawContext& ctx) {  // src/vk_engine.cpp:1716-1736
  mat4 node_matrix = svrm::mul(world_transform, top_matrix);     // world * top, as written there
  for (size_t si = 0; si < mesh->surfaces.size(); si++) {
    const GeoSurface& s = mesh->surfaces[si];
    SvrRenderObject obj{};
    obj.material = s.material->handle;
    obj.index_count = s.count;
    obj.first_index = s.startIndex;
    obj.mesh = mesh->meshBuffers;
    obj.bounds = s.bounds;
    std::memcpy(obj.transform, node_matrix.data(), 64);
    if (s.material->pass_type == SVR_PASS_TRANSPARENT)
      ctx.transparent_surfaces.push_back(obj);
    else {
      ctx.opaque_surfaces.push_back(obj);
      ctx.opaque_sources.emplace_back(mesh.get(), (uint32_t)si);
    }
  }
  Node::Draw(top_matrix, ctx);
}
void LoadedScene::Draw(const mat4& top_matrix, DrawContext& ctx) {  // src/vk_loader.cpp:56-60
  for (auto& n : top_nodes) n->Draw(top_matrix, ctx);
}

SvrBounds loader_bounds(const std::vector<SvrVertex>& v, size_t initial_vtx) {  // src/vk_loader.cpp:366-375
  float mn[3], mx[3];
  for (int k = 0; k < 3; k++) mn[k] = mx[k] = v[initial_vtx].position[k];
  for (const SvrVertex& vert : v)
    for (int k = 0; k < 3; k++) {
      mn[k] = std::min(mn[k], vert.position[k]);
      mx[k] = std::max(mx[k], vert.position[k]);
    }
  SvrBounds b{};
  for (int k = 0; k < 3; k++) {
    b.origin[k] = (mx[k] + mn[k]) / 2.f;
    b.extents[k] = (mx[k] - mn[k]) / 2.f;
  }
  b.sphere_radius = std::sqrt(b.extents[0] * b.extents[0] + b.extents[1] * b.extents[1] + b.extents[2] * b.extents[2]);
  return b;
}

// ---------------------------------------------------------------- engine
bool SvrEngine::init(const std::string& library_path, uint32_t w, uint32_t h) {
  window_width = w;
  window_height = h;
  svrm::render_extent(w, h, render_scale, &width, &height);  // src/vk_engine.cpp:1220-1222
  if (!api.load(library_path, &error)) return false;
  if (upscale && !(api.svr_upscale_to_swapchain && api.svr_read_upscaled)) {
    error = "--upscale: the library has no upscaled present (include/svr_upscale.h)";
    return false;
  }
  SvrConfig cfg{};
  cfg.width = width;
  cfg.height = height;
  cfg.color_format = SVR_COLOR_RGBA16F;  // _draw_image format, src/vk_engine.cpp:749
  cfg.device = device;
  if (api.svr_create(&cfg, &ctx)) {
    error = api.svr_last_error();
    return false;
  }
  // init_default_data, src/vk_engine.cpp:226-283: bytes are R,G,B,A in memory (__builtin_bswap32)
  const uint8_t white[4] = {0xFF, 0xFF, 0xFF, 0xFF}, grey[4] = {0xAA, 0xAA, 0xAA, 0xFF}, black[4] = {0, 0, 0, 0xFF};
  white_image = create_image(white, 1, 1, false);
  grey_image = create_image(grey, 1, 1, false);
  black_image = create_image(black, 1, 1, false);
  std::vector<uint8_t> pixels(32 * 32 * 4);
  for (int x = 0; x < 32; x++)
    for (int y = 0; y < 32; y++) {
      bool magenta = ((x % 2) ^ (y % 2)) != 0;
      uint8_t* p = &pixels[(y * 32 + x) * 4];
      p[0] = magenta ? 0xFF : 0;
      p[1] = 0;
      p[2] = magenta ? 0xFF : 0;
      p[3] = 0xFF;
    }
  error_checkerboard_image = create_image(pixels.data(), 32, 32, false);
  SvrSamplerDesc sampl{};  // zero-initialised VkSamplerCreateInfo: mip NEAREST, lods 0
  sampl.mag_filter = sampl.min_filter = SVR_FILTER_NEAREST;
  api.svr_create_sampler(ctx, &sampl, &default_sampler_nearest);
  sampl.mag_filter = sampl.min_filter = SVR_FILTER_LINEAR;
  api.svr_create_sampler(ctx, &sampl, &default_sampler_linear);
  const float ones[4] = {1, 1, 1, 1};
  auto m = write_material(SVR_PASS_MAIN_COLOR, ones, white_image, default_sampler_linear);
  if (!m) return false;
  default_data = *m;
  init_camera();
  return white_image && error_checkerboard_image;
}

void SvrEngine::cleanup() {
  release_views();
  if (ctx && draw_list && api.svr_destroy_draw_list) api.svr_destroy_draw_list(ctx, draw_list);
  draw_list = 0;
  if (ctx && pyramid && api.svr_destroy_depth_pyramid) api.svr_destroy_depth_pyramid(ctx, pyramid);
  pyramid = 0;
  if (ctx) api.svr_destroy(ctx);
  ctx = nullptr;
  api.unload();
}

void SvrEngine::init_camera() {  // src/vk_engine.cpp:203-210
  main_camera.velocity = vec3{0, 0, 0};
  main_camera.position = vec3{30.f, 0.f, -85.f};
  main_camera.pitch = 0.f;
  main_camera.yaw = 0.f;
}

SvrMesh SvrEngine::upload_mesh(const std::vector<uint32_t>& indices, const std::vector<SvrVertex>& vertices) {
  SvrMesh h = 0;
  if (api.svr_upload_mesh(ctx, indices.data(), indices.size(), vertices.data(), vertices.size(), &h)) error = api.svr_last_error();
  return h;
}
SvrImage SvrEngine::create_image(const void* rgba8, uint32_t w, uint32_t h, bool mipmapped) {
  SvrImage img = 0;
  if (api.svr_create_image(ctx, rgba8, w, h, mipmapped ? 1 : 0, &img)) error = api.svr_last_error();
  return img;
}
std::shared_ptr<MaterialInstance> SvrEngine::write_material(int pass, const float color_factors[4], SvrImage image,
                                                            SvrSampler sampler) {
  const float mr[4] = {1.f, 0.5f, 0.f, 0.f};  // src/vk_engine.cpp:275
  auto m = std::make_shared<MaterialInstance>();
  m->pass_type = pass;
  if (api.svr_write_material(ctx, pass, color_factors, mr, image, sampler, &m->handle)) {
    error = api.svr_last_error();
    return nullptr;
  }
  return m;
}

void SvrEngine::update_scene() {  // src/vk_engine.cpp:1479-1512
  auto t0 = std::chrono::system_clock::now();
  main_draw_context.opaque_surfaces.clear();
  main_draw_context.opaque_sources.clear();
  main_camera.update();
  mat4 view = main_camera.get_view_matrix();
  for (auto& kv : loaded_scenes) kv.second->Draw(svrm::identity(), main_draw_context);
  mat4 proj = svrm::perspective(svrm::radians(70.f), (float)width / (float)height, 10000.f, 0.1f);
  proj.m[1][1] *= -1;
  mat4 viewproj = svrm::mul(proj, view);
  if (taa_blend > 0.f) {  // --taa: the frame is drawn with a sub-pixel shift, the reprojection uses the unshifted matrices
    taa_viewproj = viewproj;
    const unsigned i = taa_frame % 16u + 1u;
    proj = svrm::jitter_projection(proj, svrm::halton(i, 2) - 0.5f, svrm::halton(i, 3) - 0.5f, (float)width, (float)height);
    viewproj = svrm::mul(proj, view);
  }
  std::memcpy(scene_data.view, view.data(), 64);
  std::memcpy(scene_data.proj, proj.data(), 64);
  std::memcpy(scene_data.viewproj, viewproj.data(), 64);
  for (int k = 0; k < 4; k++) {
    scene_data.ambient_color[k] = 0.1f;
    scene_data.sunlight_color[k] = 1.f;
  }
  const float dir[4] = {0, 1, 0.5f, 1.f};
  std::memcpy(scene_data.sunlight_direction, dir, 16);
  auto t1 = std::chrono::system_clock::now();
  stats.scene_update_time = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count() / 1000.f;
}

bool SvrEngine::draw_background() {  // src/vk_engine.cpp:1341-1355: dispatch the current ComputeEffect
  if (background_effects.empty()) {  // init_background_pipelines, src/vk_engine.cpp:977-989
    ComputeEffect gradient, sky;
    gradient.name = "gradient";
    gradient.effect = SVR_BACKGROUND_GRADIENT;
    for (int k = 0; k < 8; k++) gradient.data[k] = 1.0f;
    sky.name = "sky";
    sky.effect = SVR_BACKGROUND_SKY;
    sky.data[0] = 0.1f; sky.data[1] = 0.2f; sky.data[2] = 0.4f; sky.data[3] = 0.97f;
    background_effects.push_back(gradient);
    background_effects.push_back(sky);
  }
  const ComputeEffect& effect = background_effects[(size_t)current_background_effect % background_effects.size()];
  if (api.svr_draw_background(ctx, effect.effect, effect.data)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::read_swapchain(std::vector<uint8_t>& out) {
  uint32_t sw = swapchain_width ? swapchain_width : window_width, sh = swapchain_height ? swapchain_height : window_height;
  out.resize((size_t)sw * sh * 4);
  const SvrUpscalePass up = {upscale_sharpness, 0u};
  if (upscale ? api.svr_read_upscaled(ctx, &up, sw, sh, SVR_SWAPCHAIN_B8G8R8A8, out.data(), out.size())
              : api.svr_read_swapchain(ctx, sw, sh, SVR_SWAPCHAIN_B8G8R8A8, out.data(), out.size())) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

static bool same_objects(const SvrRenderObject& a, const SvrRenderObject& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

bool SvrEngine::sync_draw_list() {
  if (!api.svr_create_draw_list) {
    error = "--retained: this library has no draw lists (include/svr_draw_list.h)";
    return false;
  }
  const DrawContext& now = main_draw_context;
  DrawContext& held = list_context;
  const size_t n_op = now.opaque_surfaces.size(), n_all = n_op + now.transparent_surfaces.size();
  auto at = [&](const DrawContext& c, size_t i) -> const SvrRenderObject& {
    return i < c.opaque_surfaces.size() ? c.opaque_surfaces[i] : c.transparent_surfaces[i - c.opaque_surfaces.size()];
  };
  if (draw_list && held.opaque_surfaces.size() == n_op && held.transparent_surfaces.size() == n_all - n_op) {
    size_t first = 0, last = n_all;  // the run [first, last) that changed
    while (first < n_all && same_objects(at(now, first), at(held, first))) first++;
    while (last > first && same_objects(at(now, last - 1), at(held, last - 1))) last--;
    if (first == last) return true;  // the usual frame: nothing to do
    std::vector<SvrRenderObject> run;
    for (size_t i = first; i < last; i++) run.push_back(at(now, i));
    if (api.svr_update_draw_list(ctx, draw_list, first, run.data(), run.size())) {
      error = api.svr_last_error();
      return false;
    }
  } else {
    if (draw_list) api.svr_destroy_draw_list(ctx, draw_list);
    draw_list = 0;
    if (api.svr_create_draw_list(ctx, now.opaque_surfaces.data(), n_op, now.transparent_surfaces.data(), n_all - n_op, &draw_list)) {
      error = api.svr_last_error();
      return false;
    }
  }
  held.opaque_surfaces = now.opaque_surfaces;
  held.transparent_surfaces = now.transparent_surfaces;
  return true;
}

bool SvrEngine::occlusion_begin() {
  if (occlusion == Occlusion::Off) return true;
  if (!api.svr_create_depth_pyramid || !api.svr_destroy_depth_pyramid || !api.svr_build_depth_pyramid ||
      !api.svr_set_occlusion_pyramid) {
    error = "--occlusion: the library has no occlusion culling (include/svr_occlusion.h)";
    return false;
  }
  if (!pyramid && api.svr_create_depth_pyramid(ctx, &pyramid)) {
    error = api.svr_last_error();
    return false;
  }
  if (occlusion == Occlusion::Prepass) {  // the occluders' depth, with this frame's camera, then its pyramid
    std::vector<SvrRenderObject> occ;
    for (const SvrRenderObject& o : main_draw_context.opaque_surfaces)
      for (SvrMaterial m : occluder_materials)
        if (o.material == m) {
          occ.push_back(o);
          break;
        }
    SvrStats st{};
    if (api.svr_set_occlusion_pyramid(ctx, 0) || api.svr_draw_depth(ctx, &scene_data, occ.data(), occ.size(), &st) ||
        api.svr_build_depth_pyramid(ctx, pyramid, nullptr)) {
      error = api.svr_last_error();
      return false;
    }
  }
  if (api.svr_set_occlusion_pyramid(ctx, pyramid)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::occlusion_end() {
  if (occlusion != Occlusion::Last) return true;
  if (api.svr_build_depth_pyramid(ctx, pyramid, nullptr)) {  // this frame's depth: the next frame culls against it
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::draw_geometry() {  // src/vk_engine.cpp:1357-1477: the whole body is one call
  SvrStats st{};
  int rc;
  if (!occlusion_begin()) return false;
  if (retained) {
    if (!sync_draw_list()) return false;
    rc = api.svr_draw_list(ctx, draw_list, &scene_data, &st);  // the three counts arrive with the pass (svr_get_stats)
  } else {
    rc = api.svr_draw_geometry(ctx, &scene_data, main_draw_context.opaque_surfaces.data(),
                               main_draw_context.opaque_surfaces.size(), main_draw_context.transparent_surfaces.data(),
                               main_draw_context.transparent_surfaces.size(), &st);
  }
  if (rc) {
    error = api.svr_last_error();
    return false;
  }
  if (!occlusion_end()) return false;
  stats.drawcall_count = st.drawcall_count;
  stats.triangle_count = st.triangle_count;
  stats.mesh_draw_time = st.mesh_draw_time;
  main_draw_context.opaque_surfaces.clear();
  main_draw_context.transparent_surfaces.clear();
  // the IDs of this pass count its opaque list as given (a draw list's too: sync_draw_list made it the list's order)
  drawn_sources.swap(main_draw_context.opaque_sources);
  main_draw_context.opaque_sources.clear();
  return true;
}

bool SvrEngine::draw_depth() {  // draw_geometry without shading: a shadow or depth pass at the same call site
  if (!api.svr_draw_depth || !api.svr_draw_list_depth) {
    error = "--depth-only: the library has no depth-only passes (include/svr_depth.h)";
    return false;
  }
  SvrStats st{};
  int rc;
  if (!occlusion_begin()) return false;
  if (retained) {
    if (!sync_draw_list()) return false;
    rc = api.svr_draw_list_depth(ctx, draw_list, &scene_data, &st);
  } else {
    rc = api.svr_draw_depth(ctx, &scene_data, main_draw_context.opaque_surfaces.data(), main_draw_context.opaque_surfaces.size(), &st);
  }
  if (rc) {
    error = api.svr_last_error();
    return false;
  }
  if (!occlusion_end()) return false;
  stats.drawcall_count = st.drawcall_count;
  stats.triangle_count = st.triangle_count;
  stats.mesh_draw_time = st.mesh_draw_time;
  main_draw_context.opaque_surfaces.clear();
  main_draw_context.transparent_surfaces.clear();
  drawn_sources.swap(main_draw_context.opaque_sources);
  main_draw_context.opaque_sources.clear();
  return true;
}

bool SvrEngine::post_pass(const SvrPostPass& pass) {
  if (!api.svr_post_pass) {
    error = "--post: the library has no post pass (include/svr_post.h)";
    return false;
  }
  if (api.svr_post_pass(ctx, &pass)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::reflect_pass(float intensity, float max_distance, uint32_t steps, uint32_t frame_index) {
  if (!api.svr_reflect_pass) {
    error = "--reflect: the library has no reflection pass (include/svr_reflect.h)";
    return false;
  }
  SvrReflectPass rp{};
  mat4 viewproj, proj;
  std::memcpy(viewproj.data(), scene_data.viewproj, 64);
  std::memcpy(proj.data(), scene_data.proj, 64);
  const mat4 inv = svrm::inverse(viewproj);
  std::memcpy(rp.viewproj, viewproj.data(), 64);
  std::memcpy(rp.inv_viewproj, inv.data(), 64);
  rp.camera_position[0] = main_camera.position.x;
  rp.camera_position[1] = main_camera.position.y;
  rp.camera_position[2] = main_camera.position.z;
  svrm::dof_depth_terms(proj, &rp.inv_z_scale, &rp.inv_z_bias);
  rp.max_distance = max_distance;
  rp.steps = steps;
  rp.refine = 4;
  rp.thickness = 0.1f;
  rp.f0 = 0.04f;
  rp.intensity = intensity;
  rp.distance_fade = 1.f;
  rp.edge_width = 16.f;
  rp.resolve = 1;
  rp.depth_tolerance = 0.05f;
  rp.frame_index = frame_index;
  last_reflect = rp;
  if (api.svr_reflect_pass(ctx, &rp)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::read_attribute(int attr, std::vector<float>& out) {
  if (!api.svr_read_attribute) {
    error = "the library has no attribute targets (include/svr_attributes.h)";
    return false;
  }
  out.resize((size_t)width * height * 4);
  if (api.svr_read_attribute(ctx, attr, out.data(), out.size() * 4)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::fog_pass(float density, float falloff, float anisotropy, uint32_t frame_index) {
  if (!api.svr_fog_pass) {
    error = "--fog: the library has no fog pass (include/svr_fog.h)";
    return false;
  }
  SvrFogPass fp{};
  mat4 viewproj;
  std::memcpy(viewproj.data(), scene_data.viewproj, 64);
  const mat4 inv = svrm::inverse(viewproj);
  std::memcpy(fp.inv_viewproj, inv.data(), 64);
  fp.camera_position[0] = main_camera.position.x;
  fp.camera_position[1] = main_camera.position.y;
  fp.camera_position[2] = main_camera.position.z;
  fp.density = density;
  fp.height_falloff = falloff;
  fp.height_base = 0.f;
  fp.max_distance = 200.f;
  fp.steps = 16;
  fp.anisotropy = anisotropy;
  std::memcpy(fp.sunlight_direction, scene_data.sunlight_direction, 16);
  for (int k = 0; k < 3; k++) {
    fp.fog_color[k] = scene_data.ambient_color[k];
    fp.sun_color[k] = scene_data.sunlight_color[k] * scene_data.sunlight_color[3];
  }
  fp.edge_sharpness = 1.f;
  fp.frame_index = frame_index;
  last_fog = fp;
  if (api.svr_fog_pass(ctx, &fp)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::dof_pass(float focus_distance, float blur_scale, float max_radius) {
  if (!api.svr_dof_pass) {
    error = "--dof: the library has no depth of field pass (include/svr_dof.h)";
    return false;
  }
  SvrDofPass dp{};
  mat4 proj;
  std::memcpy(proj.data(), scene_data.proj, 64);
  svrm::dof_depth_terms(proj, &dp.inv_z_scale, &dp.inv_z_bias);
  dp.focus_distance = focus_distance;
  dp.blur_scale = blur_scale;
  dp.max_radius = max_radius;
  last_dof = dp;
  if (api.svr_dof_pass(ctx, &dp)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::motion_blur_pass(float shutter, float yaw_degrees, float max_blur) {
  if (!api.svr_motion_blur_pass) {
    error = "--motion-blur: the library has no motion blur pass (include/svr_motion.h)";
    return false;
  }
  SvrMotionBlurPass mp{};
  // update_scene's matrices without the jitter, for this frame's camera and for the one turned by yaw_degrees
  mat4 proj = svrm::perspective(svrm::radians(70.f), (float)width / (float)height, 10000.f, 0.1f);
  proj.m[1][1] *= -1;
  Camera prev = main_camera;
  prev.yaw += svrm::radians(yaw_degrees);
  const mat4 m = svrm::temporal_reproject(svrm::mul(proj, prev.get_view_matrix()), svrm::mul(proj, main_camera.get_view_matrix()));
  std::memcpy(mp.reproject, m.data(), 64);
  mp.shutter = shutter;
  mp.max_blur = max_blur;
  last_motion = mp;
  if (api.svr_motion_blur_pass(ctx, &mp)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::meter_exposure(float key, float adapt) {
  if (!api.svr_meter_exposure || !api.svr_set_post_auto_exposure) {
    error = "--auto-exposure: the library has no auto-exposure (include/svr_exposure.h)";
    return false;
  }
  if (!auto_exposure_on && api.svr_set_post_auto_exposure(ctx, 1)) {
    error = api.svr_last_error();
    return false;
  }
  auto_exposure_on = true;
  const SvrExposureMeter m{key, 0.0f, 1.0f, 0x1p-10f, 0x1p10f, adapt};
  if (api.svr_meter_exposure(ctx, &m)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::read_exposure(SvrExposureState& out) {
  if (!api.svr_read_exposure) {
    error = "--auto-exposure: the library has no auto-exposure (include/svr_exposure.h)";
    return false;
  }
  if (api.svr_read_exposure(ctx, &out)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::temporal_resolve() {
  if (!api.svr_temporal_resolve) {
    error = "--taa: the library has no temporal pass (include/svr_temporal.h)";
    return false;
  }
  SvrTemporalPass tp{};
  const mat4 m = taa_has_prev ? svrm::temporal_reproject(taa_prev_viewproj, taa_viewproj) : svrm::identity();
  std::memcpy(tp.reproject, m.data(), 64);
  tp.blend = taa_blend;
  if (api.svr_temporal_resolve(ctx, &tp)) {
    error = api.svr_last_error();
    return false;
  }
  taa_prev_viewproj = taa_viewproj;
  taa_has_prev = true;
  taa_frame++;
  return true;
}

bool SvrEngine::draw_deferred() {  // draw_geometry in three steps: G-buffer pass, lighting pass, transparent objects over it
  if (!api.svr_enable_attributes || !api.svr_light_pass || !api.svr_set_depth_load_op) {
    error = "--deferred: the library has no attribute targets, lighting pass or depth loadOp (include/svr_attributes.h, svr_lighting.h, svr_load.h)";
    return false;
  }
  if (!gbuffer && api.svr_enable_attributes(ctx, SVR_ATTR_NORMAL | SVR_ATTR_ALBEDO)) {
    error = api.svr_last_error();
    return false;
  }
  gbuffer = true;
  const DrawContext& dc = main_draw_context;
  SvrStats st{}, st_tr{};
  SvrLightPass lp{};
  mat4 viewproj;
  std::memcpy(viewproj.data(), scene_data.viewproj, 64);
  const mat4 inv = svrm::inverse(viewproj);
  std::memcpy(lp.inv_viewproj, inv.data(), 64);
  std::memcpy(lp.ambient_color, scene_data.ambient_color, 16);
  std::memcpy(lp.sunlight_direction, scene_data.sunlight_direction, 16);
  std::memcpy(lp.sunlight_color, scene_data.sunlight_color, 16);
  int rc = api.svr_draw_geometry(ctx, &scene_data, dc.opaque_surfaces.data(), dc.opaque_surfaces.size(), nullptr, 0, &st);
  if (!rc && ao_radius > 0.f) {  // --ao: the ambient factor of this frame's G-buffer, used by the lighting pass below
    if (!api.svr_ambient_pass || !api.svr_set_light_ambient_occlusion) {
      error = "--ao: the library has no ambient pass (include/svr_ambient.h)";
      return false;
    }
    SvrAmbientPass ap{};
    std::memcpy(ap.inv_viewproj, inv.data(), 64);
    mat4 proj;
    std::memcpy(proj.data(), scene_data.proj, 64);
    ap.radius = ao_radius;
    ap.pixels_per_unit = svrm::pixels_per_unit(proj, (float)height);
    ap.bias = 0.02f * ao_radius;
    ap.intensity = ao_intensity;
    ap.sharpness = 0.05f;
    rc = api.svr_ambient_pass(ctx, &ap);
    if (!rc) rc = api.svr_set_light_ambient_occlusion(ctx, 1);
  }
  if (!rc) rc = api.svr_light_pass(ctx, &lp);
  if (!rc) rc = api.svr_set_depth_load_op(ctx, SVR_DEPTH_LOAD);
  if (!rc) {
    rc = api.svr_draw_geometry(ctx, &scene_data, nullptr, 0, dc.transparent_surfaces.data(), dc.transparent_surfaces.size(), &st_tr);
    if (rc) error = api.svr_last_error();
    if (api.svr_set_depth_load_op(ctx, SVR_DEPTH_CLEAR) && !rc) rc = SVR_ERR_DEVICE;
  }
  if (rc) {
    if (error.empty()) error = api.svr_last_error();
    return false;
  }
  stats.drawcall_count = st.drawcall_count + st_tr.drawcall_count;
  stats.triangle_count = st.triangle_count + st_tr.triangle_count;
  stats.mesh_draw_time = st.mesh_draw_time + st_tr.mesh_draw_time;
  main_draw_context.opaque_surfaces.clear();
  main_draw_context.transparent_surfaces.clear();
  drawn_sources.swap(main_draw_context.opaque_sources);
  main_draw_context.opaque_sources.clear();
  return true;
}

bool SvrEngine::enable_ids() {
  if (!api.svr_enable_ids || !api.svr_pick) {
    error = "this library has no ID target (include/svr_ids.h)";
    return false;
  }
  if (api.svr_enable_ids(ctx, 1)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

bool SvrEngine::pick(uint32_t x, uint32_t y, Pick& out) {
  out = Pick{};
  uint32_t id[2] = {0, 0};
  if (!api.svr_pick || api.svr_pick(ctx, x, y, id)) {
    error = api.svr_pick ? api.svr_last_error() : "this library has no ID target (include/svr_ids.h)";
    return false;
  }
  if (id[0] == 0) return true;
  if (id[0] > drawn_sources.size()) {
    error = "pick: object " + std::to_string(id[0]) + " beyond the frame's " + std::to_string(drawn_sources.size()) + " opaque objects";
    return false;
  }
  const auto& src = drawn_sources[id[0] - 1];
  out.hit = true;
  out.object = id[0];
  out.primitive = id[1];
  out.mesh = src.first->name;
  out.surface = src.second;
  return true;
}

bool SvrEngine::draw() {  // src/vk_engine.cpp:1218-1339 minus acquire/blit/ImGui/present
  update_scene();
  if (!draw_background()) return false;
  if (!draw_geometry()) return false;
  frame_number++;
  return true;
}

bool SvrEngine::read_color_rgba16f(std::vector<uint16_t>& out) {
  out.resize((size_t)width * height * 4);
  if (api.svr_read_color(ctx, out.data(), out.size() * 2, 0)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}
bool SvrEngine::read_depth(std::vector<float>& out) {
  out.resize((size_t)width * height);
  if (api.svr_read_depth(ctx, out.data(), out.size() * 4)) {
    error = api.svr_last_error();
    return false;
  }
  return true;
}

}  // namespace svrhost

// ---------------------------------------------------------------- multiview (include/svr_views.h)
namespace svrhost {
namespace {
// the device allocator and copies of the HIP runtime the product library already has loaded (this harness has no HIP
// of its own): hipMalloc / hipFree / hipMemcpy by name
struct HipRt {
  int (*malloc_)(void**, size_t) = nullptr;
  int (*free_)(void*) = nullptr;
  int (*memcpy_)(void*, const void*, size_t, int) = nullptr;
  bool load() {
    if (malloc_) return true;
    void* h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("libamdhip64.so", RTLD_NOW);
    if (!h) return false;
    malloc_ = reinterpret_cast<decltype(malloc_)>(dlsym(h, "hipMalloc"));
    free_ = reinterpret_cast<decltype(free_)>(dlsym(h, "hipFree"));
    memcpy_ = reinterpret_cast<decltype(memcpy_)>(dlsym(h, "hipMemcpy"));
    return malloc_ && free_ && memcpy_;
  }
};
HipRt g_hip;
constexpr int HIP_H2D = 1, HIP_D2H = 2;
}  // namespace

float SvrEngine::view_yaw(uint32_t k) const { return main_camera.yaw + (float)k * (svrm::radians(360.f) / (float)views); }

bool SvrEngine::draw_geometry_views() {
  if (!api.svr_draw_geometry_views || !api.svr_draw_list_views) {
    error = "--views: the library has no multiview (include/svr_views.h)";
    return false;
  }
  const size_t px = (size_t)width * height;
  if (!view_color) {
    if (!g_hip.load()) {
      error = "--views: no HIP runtime to allocate the layers";
      return false;
    }
    if (g_hip.malloc_(&view_color, px * 8 * views) || g_hip.malloc_((void**)&view_depth, px * 4 * views)) {
      error = "--views: hipMalloc failed";
      return false;
    }
  }
  // every layer starts as the context's target after the background: what a single-camera frame loads
  std::vector<uint16_t> bg(px * 4);
  if (api.svr_read_color(ctx, bg.data(), bg.size() * 2, 0)) {
    error = api.svr_last_error();
    return false;
  }
  for (uint32_t k = 0; k < views; k++)
    if (g_hip.memcpy_((char*)view_color + px * 8 * k, bg.data(), px * 8, HIP_H2D)) {
      error = "--views: hipMemcpy failed";
      return false;
    }
  // the cameras: update_scene's matrices with the yaw of view k
  std::vector<SvrSceneData> scenes(views, scene_data);
  for (uint32_t k = 0; k < views; k++) {
    Camera cam = main_camera;
    cam.yaw = view_yaw(k);
    mat4 view = cam.get_view_matrix();
    mat4 proj = svrm::perspective(svrm::radians(70.f), (float)width / (float)height, 10000.f, 0.1f);
    proj.m[1][1] *= -1;
    mat4 viewproj = svrm::mul(proj, view);
    std::memcpy(scenes[k].view, view.data(), 64);
    std::memcpy(scenes[k].proj, proj.data(), 64);
    std::memcpy(scenes[k].viewproj, viewproj.data(), 64);
  }
  SvrViewTargets t{};
  t.color = view_color;
  t.depth = view_depth;
  SvrStats st{};
  int rc;
  if (retained) {
    if (!sync_draw_list()) return false;
    rc = api.svr_draw_list_views(ctx, draw_list, views, scenes.data(), &t, &st);
  } else {
    rc = api.svr_draw_geometry_views(ctx, views, scenes.data(), &t, main_draw_context.opaque_surfaces.data(),
                                     main_draw_context.opaque_surfaces.size(), main_draw_context.transparent_surfaces.data(),
                                     main_draw_context.transparent_surfaces.size(), &st);
  }
  if (rc) {
    error = api.svr_last_error();
    return false;
  }
  stats.drawcall_count = st.drawcall_count;
  stats.triangle_count = st.triangle_count;
  stats.mesh_draw_time = st.mesh_draw_time;
  // as after draw_geometry: update_scene refills the opaque list only, the transparent one is emptied here
  main_draw_context.opaque_surfaces.clear();
  main_draw_context.transparent_surfaces.clear();
  drawn_sources.swap(main_draw_context.opaque_sources);
  main_draw_context.opaque_sources.clear();
  return true;
}

void SvrEngine::release_views() {
  if (ctx && view_color) api.svr_sync(ctx);  // passes in flight write the layers
  if (view_color) g_hip.free_(view_color);
  if (view_depth) g_hip.free_(view_depth);
  view_color = nullptr;
  view_depth = nullptr;
}

bool SvrEngine::read_view_layers(std::vector<uint16_t>& color, std::vector<float>& depth) {
  const size_t px = (size_t)width * height;
  if (api.svr_sync(ctx)) {
    error = api.svr_last_error();
    return false;
  }
  color.resize(px * 4 * views);
  depth.resize(px * views);
  if (g_hip.memcpy_(color.data(), view_color, color.size() * 2, HIP_D2H) || g_hip.memcpy_(depth.data(), view_depth, depth.size() * 4, HIP_D2H)) {
    error = "--views: hipMemcpy failed";
    return false;
  }
  return true;
}

// ---------------------------------------------------------------- the stats window (include/svr_overlay.h)
bool SvrEngine::stats_overlay(std::vector<uint8_t>& image, std::string& drawn) {
  if (!api.svr_draw_overlay || !api.svr_overlay_font) {
    error = "--stats-overlay: the library has no overlay pass (include/svr_overlay.h)";
    return false;
  }
  if (!g_hip.load()) {
    error = "--stats-overlay: no HIP runtime to allocate the swapchain image";
    return false;
  }
  const uint32_t sw = swapchain_width ? swapchain_width : window_width, sh = swapchain_height ? swapchain_height : window_height;
  const uint8_t* atlas = nullptr;
  uint32_t aw = 0, ah = 0, cw = 0, ch = 0, first = 0, n = 0;
  api.svr_overlay_font(&atlas, &aw, &ah, &cw, &ch, &first, &n);
  void *d_image = nullptr, *d_atlas = nullptr;
  bool ok = false;
  do {
    if (g_hip.malloc_(&d_image, (size_t)sw * sh * 4) || g_hip.malloc_(&d_atlas, (size_t)aw * ah) || g_hip.memcpy_(d_atlas, atlas, (size_t)aw * ah, HIP_H2D)) {
      error = "--stats-overlay: hipMalloc or hipMemcpy failed";
      break;
    }
    // src/vk_engine.cpp:1276, or the upscaled present in its place (include/svr_upscale.h)
    const SvrUpscalePass up = {upscale_sharpness, 0u};
    if (upscale ? api.svr_upscale_to_swapchain(ctx, &up, d_image, sw, sh, SVR_SWAPCHAIN_B8G8R8A8) : api.svr_copy_to_swapchain(ctx, d_image, sw, sh, SVR_SWAPCHAIN_B8G8R8A8)) {
      error = api.svr_last_error();
      break;
    }
    // draw_imgui (src/vk_engine.cpp:1282): the stats window of src/vk_engine.cpp:1186-1190
    OverlayListBuilder b(aw, ah, cw, ch, first, n);
    static const uint8_t ink[4] = {255, 255, 255, 255};
    char line[5][96];
    snprintf(line[0], sizeof(line[0]), "frametime %f ms", (double)stats.frame_time);
    snprintf(line[1], sizeof(line[1]), "draw time %f ms", (double)stats.mesh_draw_time);
    snprintf(line[2], sizeof(line[2]), "update time %f ms", (double)stats.scene_update_time);
    snprintf(line[3], sizeof(line[3]), "triangles %i", stats.triangle_count);
    snprintf(line[4], sizeof(line[4]), "draws %i", stats.drawcall_count);
    const int wx = 10, wy = 10, ww = 150, wh = 64;
    b.window((float)wx, (float)wy, (float)ww, (float)wh, "stats");
    drawn = "window " + std::to_string(wx) + " " + std::to_string(wy) + " " + std::to_string(ww) + " " + std::to_string(wh) + " stats\n";
    for (int k = 0; k < 5; k++) {
      const int tx = wx + 4, ty = wy + 16 + 9 * k;
      b.text((float)tx, (float)ty, line[k], ink);
      drawn += "text " + std::to_string(tx) + " " + std::to_string(ty) + " " + line[k] + "\n";
    }
    const SvrOverlayTexture tex = {d_atlas, aw, ah, SVR_OVERLAY_TEX_A8, 0u};
    const SvrOverlayList list = b.list(&tex, 1);
    if (api.svr_draw_overlay(ctx, d_image, sw, sh, SVR_SWAPCHAIN_B8G8R8A8, &list) || api.svr_sync(ctx)) {
      error = api.svr_last_error();
      break;
    }
    image.resize((size_t)sw * sh * 4);
    if (g_hip.memcpy_(image.data(), d_image, image.size(), HIP_D2H)) {
      error = "--stats-overlay: hipMemcpy failed";
      break;
    }
    ok = true;
  } while (false);
  if (ctx) api.svr_sync(ctx);  // nothing in flight names the image or the atlas
  if (d_image) g_hip.free_(d_image);
  if (d_atlas) g_hip.free_(d_atlas);
  return ok;
}
}  // namespace svrhost
