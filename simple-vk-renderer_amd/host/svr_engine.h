// svr_engine.h — a VulkanEngine-shaped C++ host above the C ABI of include/svr.h.
//
// Mirrors, member for member, the parts of the reference engine that sit either side of the draw
// path, with the Vulkan plumbing replaced by svr_* calls:
//   init / cleanup / run-less frame:   src/vk_engine.cpp:171-201, 1218-1339
//   init_default_data                  src/vk_engine.cpp:226-306   (white/grey/black/checker, samplers, default material)
//   init_camera, Camera                src/vk_engine.cpp:203-210, src/camera.cpp:8-11, 54-66
//   upload_mesh / create_image         src/vk_engine.cpp:340-390, 1571-1612
//   update_scene                       src/vk_engine.cpp:1479-1512
//   draw_geometry                      src/vk_engine.cpp:1357-1477  -> one svr_draw_geometry call
//   Node / MeshNode / LoadedGLTF::Draw src/vk_types.h:146-170, src/vk_engine.cpp:1716-1736, src/vk_loader.cpp:56-60
// The library is opened with dlopen so the same harness drives the HIP product or, in tests, the oracle.
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/svr_draw_list.h"
#include "../../include/svr_ids.h"
#include "../../include/svr_depth.h"
#include "../../include/svr_lighting.h"
#include "../../include/svr_load.h"
#include "../../include/svr_occlusion.h"
#include "../../include/svr_post.h"
#include "../../include/svr_temporal.h"
#include "../../include/svr_ambient.h"
#include "../../include/svr_exposure.h"
#include "../../include/svr_fog.h"
#include "../../include/svr_dof.h"
#include "../../include/svr_motion.h"
#include "../../include/svr_reflect.h"
#include "../../include/svr_overlay.h"
#include "../../include/svr_upscale.h"
#include "../../include/svr_views.h"
#include "svr_math.h"

namespace svrhost {

using svrm::mat4;
using svrm::vec3;

// every svr.h entry point the harness uses, resolved from one shared library
struct SvrApi {
  void* handle = nullptr;
#define SVR_FN(name) decltype(&::name) name = nullptr;
  SVR_FN(svr_create) SVR_FN(svr_destroy) SVR_FN(svr_upload_mesh) SVR_FN(svr_create_image) SVR_FN(svr_create_sampler)
  SVR_FN(svr_write_material) SVR_FN(svr_clear_color) SVR_FN(svr_draw_geometry) SVR_FN(svr_sync) SVR_FN(svr_read_color)
  SVR_FN(svr_read_depth) SVR_FN(svr_get_stats) SVR_FN(svr_last_error) SVR_FN(svr_backend_name)
  SVR_FN(svr_draw_background) SVR_FN(svr_read_swapchain) SVR_FN(svr_copy_to_swapchain) SVR_FN(svr_set_option)
  // include/svr_draw_list.h: optional (the HIP library has them, the oracle does not); needed by SvrEngine::retained
  SVR_FN(svr_create_draw_list) SVR_FN(svr_update_draw_list) SVR_FN(svr_destroy_draw_list) SVR_FN(svr_draw_list)
  // include/svr_ids.h: optional as well (HIP library only); needed by SvrEngine::pick
  SVR_FN(svr_enable_ids) SVR_FN(svr_pick)
  // include/svr_views.h: optional (HIP library only), needed by SvrEngine::draw_views
  SVR_FN(svr_draw_geometry_views) SVR_FN(svr_draw_list_views)
  // include/svr_depth.h: optional (HIP library only), needed by SvrEngine::draw_depth
  SVR_FN(svr_draw_depth) SVR_FN(svr_draw_list_depth)
  // include/svr_occlusion.h: optional (HIP library only), needed by SvrEngine::occlusion
  SVR_FN(svr_create_depth_pyramid) SVR_FN(svr_destroy_depth_pyramid) SVR_FN(svr_build_depth_pyramid)
  SVR_FN(svr_set_occlusion_pyramid)
  // include/svr_attributes.h, svr_lighting.h and svr_load.h: optional (HIP library only), needed by SvrEngine::draw_deferred
  SVR_FN(svr_enable_attributes) SVR_FN(svr_light_pass) SVR_FN(svr_set_depth_load_op)
  // include/svr_post.h: optional (HIP library only), needed by SvrEngine::post_pass
  SVR_FN(svr_post_pass)
  // include/svr_temporal.h: optional (HIP library only), needed by SvrEngine::temporal_resolve
  SVR_FN(svr_temporal_resolve)
  // include/svr_ambient.h: optional (HIP library only), needed by SvrEngine::draw_deferred with ao_radius > 0
  SVR_FN(svr_ambient_pass) SVR_FN(svr_set_light_ambient_occlusion)
  // include/svr_exposure.h: optional (HIP library only), needed by SvrEngine::meter_exposure
  SVR_FN(svr_meter_exposure) SVR_FN(svr_set_post_auto_exposure) SVR_FN(svr_read_exposure)
  // include/svr_overlay.h: optional (HIP library only), needed by SvrEngine::stats_overlay
  SVR_FN(svr_draw_overlay) SVR_FN(svr_overlay_font)
  // include/svr_upscale.h: optional (HIP library only), needed by SvrEngine::upscale
  SVR_FN(svr_upscale_to_swapchain) SVR_FN(svr_read_upscaled)
  // include/svr_fog.h: optional (HIP library only), needed by SvrEngine::fog_pass
  SVR_FN(svr_fog_pass)
  // include/svr_dof.h: optional (HIP library only), needed by SvrEngine::dof_pass
  SVR_FN(svr_dof_pass)
  // include/svr_motion.h: optional (HIP library only), needed by SvrEngine::motion_blur_pass
  SVR_FN(svr_motion_blur_pass)
  // include/svr_reflect.h: optional (HIP library only), needed by SvrEngine::reflect_pass; svr_read_attribute
  // (include/svr_attributes.h) by SvrEngine::read_attribute
  SVR_FN(svr_reflect_pass) SVR_FN(svr_read_attribute)
#undef SVR_FN
  bool load(const std::string& path, std::string* err);
  void unload();
};

struct EngineStats {  // src/vk_engine.h:16-22
  float frame_time = 0;
  int triangle_count = 0;
  int drawcall_count = 0;
  float scene_update_time = 0;
  float mesh_draw_time = 0;
};

struct Camera {  // src/camera.h:9-31 (static state there; one instance here)
  vec3 velocity, position;
  float pitch = 0.f, yaw = 0.f;
  mat4 get_view_matrix() const;
  mat4 get_rotation_matrix() const;
  void update();
};

struct MaterialInstance {  // src/vk_types.h:138-142: pipeline/descriptor set -> one handle
  SvrMaterial handle = 0;
  int pass_type = SVR_PASS_MAIN_COLOR;
};
struct GeoSurface {  // src/vk_loader.h:17-22
  uint32_t startIndex = 0, count = 0;
  SvrBounds bounds{};
  std::shared_ptr<MaterialInstance> material;
};
struct MeshAsset {  // src/vk_loader.h:24-28
  std::string name;
  std::vector<GeoSurface> surfaces;
  SvrMesh meshBuffers = 0;
};
struct DrawContext {  // src/vk_engine.h:40-43
  std::vector<SvrRenderObject> opaque_surfaces, transparent_surfaces;
  // where each opaque object came from (mesh, surface index): what an ID (include/svr_ids.h) names, object - 1
  std::vector<std::pair<const MeshAsset*, uint32_t>> opaque_sources;
};

struct Node {  // src/vk_types.h:150-170
  std::weak_ptr<Node> parent;
  std::vector<std::shared_ptr<Node>> children;
  mat4 local_transform = svrm::identity();
  mat4 world_transform = svrm::identity();
  virtual ~Node() = default;
  void refresh_transform(const mat4& parent_matrix);  // passes parent_matrix on unchanged
  virtual void Draw(const mat4& top_matrix, DrawContext& ctx);
};
struct MeshNode : Node {  // src/vk_engine.h:24-27
  std::shared_ptr<MeshAsset> mesh;
  void Draw(const mat4& top_matrix, DrawContext& ctx) override;
};
struct LoadedScene {  // LoadedGLTF, src/vk_loader.h:33-57
  std::vector<std::shared_ptr<MeshAsset>> meshes;
  std::vector<std::shared_ptr<Node>> nodes, top_nodes;
  std::vector<std::shared_ptr<MaterialInstance>> materials;
  std::vector<SvrImage> images;      // file-owned images (not the engine defaults), LoadedGLTF::images
  std::vector<SvrSampler> samplers;  // LoadedGLTF::samplers
  void Draw(const mat4& top_matrix, DrawContext& ctx);
};

struct ComputeEffect {  // src/vk_engine.h ComputeEffect: name + ComputePushConstants (4 x vec4)
  const char* name = "";
  int effect = SVR_BACKGROUND_GRADIENT;
  float data[16] = {0};
};

// GLTF loader's bounds rule (src/vk_loader.cpp:366-375): min/max start at the primitive's first vertex
// but run over every vertex accumulated in the mesh so far
SvrBounds loader_bounds(const std::vector<SvrVertex>& mesh_vertices_so_far, size_t initial_vtx);

struct SvrEngine;
// load_gltf_meshes (src/vk_loader.cpp:162-437): .glb or .gltf -> uploaded scene; nullptr + engine->error on failure
std::shared_ptr<LoadedScene> load_gltf_meshes(SvrEngine* engine, const std::string& file_path);

struct SvrEngine {
  SvrApi api;
  SvrContext* ctx = nullptr;
  uint32_t width = 1700, height = 900;  // _draw_extent: the context's extent, render_extent(window, render_scale)
  // Render scale (svr_demo --render-scale <s> [--upscale <sharpness>|off], include/svr_upscale.h): _render_scale of
  // src/vk_engine.h:121, bound.  Set before init, which takes the window's extent (_window_extent, src/vk_engine.h:219) and
  // creates the context at svrm::render_extent of it; the swapchain image stays at the window's extent.  upscale: read_swapchain
  // and stats_overlay present with svr_upscale_to_swapchain at upscale_sharpness; without it with the scaled
  // svr_copy_to_swapchain, the reference's stretch.
  float render_scale = 1.f;
  bool upscale = false;
  float upscale_sharpness = 0.5f;
  uint32_t window_width = 1700, window_height = 900;
  int device = 0;                        // SvrConfig.device: the rank's GPU in the sharded form (svr_dist.h)
  int frame_number = 0;
  EngineStats stats;
  DrawContext main_draw_context;
  SvrSceneData scene_data{};
  Camera main_camera;
  std::unordered_map<std::string, std::shared_ptr<LoadedScene>> loaded_scenes;
  // init_default_data
  SvrImage white_image = 0, grey_image = 0, black_image = 0, error_checkerboard_image = 0;
  SvrSampler default_sampler_nearest = 0, default_sampler_linear = 0;
  MaterialInstance default_data;
  std::string error;

  bool init(const std::string& library_path, uint32_t w, uint32_t h);
  void cleanup();
  SvrMesh upload_mesh(const std::vector<uint32_t>& indices, const std::vector<SvrVertex>& vertices);
  SvrImage create_image(const void* rgba8, uint32_t w, uint32_t h, bool mipmapped);
  std::shared_ptr<MaterialInstance> write_material(int pass, const float color_factors[4], SvrImage image, SvrSampler sampler);
  void init_camera();
  void update_scene();
  // init_background_pipelines (src/vk_engine.cpp:920-1000): gradient (white, white) and sky (0.1,0.2,0.4,0.97)
  std::vector<ComputeEffect> background_effects;
  int current_background_effect = 0;
  uint32_t swapchain_width = 0, swapchain_height = 0;  // _swap_chain_extent; 0 = the window's extent
  bool draw_background();
  bool draw_geometry();
  // Depth-only frames (svr_demo --depth-only 1, include/svr_depth.h): the draw context's opaque surfaces (or the draw
  // list's, retained) into the depth target without shading; the colour target keeps the background just drawn.
  bool draw_depth();
  // Deferred frames (svr_demo --deferred 1): the opaque surfaces with the NORMAL and ALBEDO planes (include/
  // svr_attributes.h), svr_light_pass with the scene's sun and ambient, no point lights and no shadow map (include/
  // svr_lighting.h), then the transparent surfaces under SVR_DEPTH_LOAD (include/svr_load.h): tested against the opaque
  // depth, blended over the lit colour.  The frame is the forward one, bit for bit.
  // With ao_radius > 0 (svr_demo --ao <radius>:<intensity>, include/svr_ambient.h) svr_ambient_pass runs between the
  // G-buffer pass and the lighting pass, and the lighting pass scales its ambient term by the plane it wrote.
  bool gbuffer = false;  // the planes are enabled
  float ao_radius = 0.f, ao_intensity = 0.f;
  bool draw_deferred();
  // The HDR post pass (svr_demo --post <operator>:<levels>, include/svr_post.h): exposure, bloom and the operator over the
  // colour target, after the frame's last pass and before the swapchain copy.
  bool post_pass(const SvrPostPass& pass);
  // The reflection pass (svr_demo --deferred 1 --reflect <intensity>:<max_distance>[:<steps>], include/svr_reflect.h): behind
  // the lighting pass and the deferred frame's transparents, in front of the fog pass.  The camera is the scene's: its
  // viewproj, the inverse of it and the main camera's position; the depth terms are those of the scene's projection
  // (svrm::dof_depth_terms).  4 bisections, thickness 0.1, f0 0.04, the weight fades to nothing at max_distance and over 16
  // pixels at the window's border, 3 x 3 resolve with a depth tolerance of 0.05.
  // last_reflect: the pass as it was handed to the library (svr_demo dumps it as <prefix>.reflect).
  SvrReflectPass last_reflect{};
  bool reflect_pass(float intensity, float max_distance, uint32_t steps, uint32_t frame_index);
  // one plane of the G-buffer, four floats per texel (svr_demo --reflect dumps <prefix>.normal and <prefix>.albedo)
  bool read_attribute(int attr, std::vector<float>& out);
  // The fog pass (svr_demo --deferred 1 --fog <density>:<falloff>[:<g>], include/svr_fog.h): behind the deferred frame's
  // transparents, in front of the temporal resolve and the post pass.  The camera is the scene's: the inverse of its
  // viewproj and the main camera's position; the sun is the scene's direction and colour (rgb times w), the fog's own
  // colour the scene's ambient; no shadow map.  height_base 0, max_distance 200, 16 steps, edge_sharpness 1.
  // last_fog: the pass as it was handed to the library (svr_demo dumps it as <prefix>.fog).
  SvrFogPass last_fog{};
  bool fog_pass(float density, float falloff, float anisotropy, uint32_t frame_index);
  // The depth of field pass (svr_demo --deferred 1 --dof <focus_distance>:<blur_scale>[:<max_radius>], include/svr_dof.h):
  // behind the fog pass, in front of the temporal resolve and the post pass.  The depth terms are those of the scene's
  // projection (svrm::dof_depth_terms; a jitter does not move them).
  // last_dof: the pass as it was handed to the library (svr_demo dumps it as <prefix>.dof).
  SvrDofPass last_dof{};
  bool dof_pass(float focus_distance, float blur_scale, float max_radius);
  // The camera motion blur pass (svr_demo --deferred 1 --motion-blur <shutter>:<yaw_degrees>[:<max_blur>],
  // include/svr_motion.h): behind the temporal resolve, in front of the meter and the post pass.  The previous frame's
  // camera is this frame's turned by yaw_degrees, so one frame is deterministic; both matrices are without jitter.
  // last_motion: the pass as it was handed to the library (svr_demo dumps it as <prefix>.motion).
  SvrMotionBlurPass last_motion{};
  bool motion_blur_pass(float shutter, float yaw_degrees, float max_blur);
  // Auto-exposure (svr_demo --auto-exposure <key>:<adapt>, include/svr_exposure.h): meter the colour target behind the
  // frame's last pass and in front of the post pass, which then multiplies its exposure (a compensation) by the state's.
  // The first call turns svr_set_post_auto_exposure on.  Whole window, exposures clamped to [2^-10, 2^10].
  bool auto_exposure_on = false;
  bool meter_exposure(float key, float adapt);
  bool read_exposure(SvrExposureState& out);
  // Temporal antialiasing (svr_demo --taa <blend>, include/svr_temporal.h).  With taa_blend > 0 update_scene shifts the
  // projection by Halton(2, 3) - 0.5 pixels, a period of 16 frames, and keeps the unjittered viewproj; temporal_resolve,
  // called behind the frame's last geometry or lighting pass and in front of the post pass, reprojects with
  // last frame's unjittered viewproj times the inverse of this frame's (the identity on the first frame).
  float taa_blend = 0.f;
  uint32_t taa_frame = 0;
  bool taa_has_prev = false;
  mat4 taa_viewproj{}, taa_prev_viewproj{};
  bool temporal_resolve();
  // Occlusion culling (svr_demo --occlusion off|last|prepass, include/svr_occlusion.h).  Last: each frame's geometry
  // culls against the pyramid of the previous frame's depth (built behind every frame; before the first it is all 0.0
  // and culls nothing).  Prepass: each frame first draws the opaque objects whose material is in occluder_materials
  // (walls, floors) as a depth-only pass, builds the pyramid from it and culls the frame against that.  Either way the
  // frames are bit for bit those without culling, for a static camera (last) or always (prepass).
  enum class Occlusion { Off, Last, Prepass };
  Occlusion occlusion = Occlusion::Off;
  std::vector<SvrMaterial> occluder_materials;
  SvrDepthPyramid pyramid = 0;
  bool occlusion_begin();  // in front of a frame's geometry pass
  bool occlusion_end();    // behind it
  // Retained mode (svr_demo --retained): the draw context goes to a draw list made once; the list is updated only
  // where the scene graph's output differs from what it holds (a changed run of objects), or made again when the
  // counts change, and every frame is one svr_draw_list.
  bool retained = false;
  SvrDrawList draw_list = 0;
  DrawContext list_context;  // what draw_list holds
  bool sync_draw_list();
  bool draw();  // update_scene -> draw_background -> draw_geometry (the present has no counterpart; draw_imgui: stats_overlay)
  // The stats window (svr_demo --stats-overlay 1, include/svr_overlay.h): what draw() does behind draw_geometry
  // (src/vk_engine.cpp:1276-1282) — the copy to a swapchain image, then draw_imgui's window with the five lines of
  // src/vk_engine.cpp:1186-1190 onto that image by svr_draw_overlay.  image: the swapchain image afterwards (B8G8R8A8);
  // drawn: the builder calls it made, a line each ("window x y w h title", "text x y string").
  bool stats_overlay(std::vector<uint8_t>& image, std::string& drawn);
  // Multiview (svr_demo --views N, include/svr_views.h): N cameras at main_camera's position, yaw stepped by 2 pi / N.
  // The layers live in device memory of the HIP runtime the library runs on; each starts as the context's colour
  // target (the background just drawn) and gets view k of the draw context, immediate or retained.
  uint32_t views = 0;
  void* view_color = nullptr;  // [views][height][width] RGBA16F texels
  float* view_depth = nullptr;
  float view_yaw(uint32_t k) const;
  bool draw_geometry_views();
  bool read_view_layers(std::vector<uint16_t>& color, std::vector<float>& depth);
  void release_views();
  // the swapchain image of the frame just drawn: vkutil::copy_image at src/vk_engine.cpp:1277 (B8G8R8A8)
  bool read_swapchain(std::vector<uint8_t>& out);
  bool read_color_rgba16f(std::vector<uint16_t>& out);
  bool read_depth(std::vector<float>& out);
  // Object picking (include/svr_ids.h): enable_ids() before the frames; pick() after one reads the pixel's ID of the last
  // frame drawn and names what won it.  hit = false where no opaque object did.
  struct Pick {
    bool hit = false;
    uint32_t object = 0, primitive = 0;  // object: the RenderObject's 1-based position in the frame's opaque list
    std::string mesh;                    // MeshAsset::name
    uint32_t surface = 0;                // index into MeshAsset::surfaces
  };
  std::vector<std::pair<const MeshAsset*, uint32_t>> drawn_sources;  // opaque_sources of the frame drawn last
  bool enable_ids();
  bool pick(uint32_t x, uint32_t y, Pick& out);
};

}  // namespace svrhost
