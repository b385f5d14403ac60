// svr_demo.cpp — drives the VulkanEngine-shaped harness (svr_engine.h) for a few frames and dumps what it
// submitted and what came back.  Used by tests/test_host_cpp.py (against the oracle on CPU, against the HIP
// library on the GPU box) and as the smallest example of the call sequence init -> load -> draw().
//
//   svr_demo --lib <libsvr_*.so> --width 160 --height 90 --frames 2 --dump /tmp/prefix [--retained 1]
//       --retained 1: the engine keeps its draw context in a draw list (include/svr_draw_list.h, HIP library only)
//       --views N: N cameras at the camera's position, yaw stepped by 360/N, in one multiview pass (include/svr_views.h,
//           HIP library only); prints "view k yaw Y" and dumps layer k as <prefix>.view<k>.color / .depth
//       --yaw Y: the camera's yaw in radians (a single-camera run of view k: --yaw <its Y>)
//       --depth-only 1: every frame's geometry is a depth-only pass (include/svr_depth.h, HIP library only): the dumped
//           depth is a normal run's, the colour the background's
//       --deferred 1: every frame is the opaque objects with normal and albedo planes, a lighting pass, then the transparent
//           objects under SVR_DEPTH_LOAD (include/svr_attributes.h, svr_lighting.h, svr_load.h; HIP library only): the
//           dumps are a normal run's
//       --post clamp|reinhard|aces:<levels> [--exposure E] [--bloom-threshold T] [--bloom-intensity I]: the HDR post pass
//           (include/svr_post.h, HIP library only) behind every frame's last pass and before the swapchain copy: the
//           .color and .swapchain dumps are taken after it
//       --reflect <intensity>:<max_distance>[:<steps>]: the reflection pass (include/svr_reflect.h, HIP library only) with
//           --deferred 1: screen-space reflections behind the lighting pass and the transparent objects, in front of --fog
//           (steps defaults to 16; 4 bisections, 3 x 3 resolve); the pass as handed to the library is dumped as
//           <prefix>.reflect, and the G-buffer's planes it read as <prefix>.normal and <prefix>.albedo.  With --taa,
//           frame_index advances per frame; without, it stays 0.  Not with --views or --ranks
//       --fog <density>:<falloff>[:<g>]: the fog pass (include/svr_fog.h, HIP library only) with --deferred 1: height fog and sun
//           shafts from the scene's sun behind the transparent objects, in front of --taa and --post (16 steps, no shadow
//           map); the pass as handed to the library is dumped as <prefix>.fog.  With --taa, frame_index advances per
//           frame, so the resolve averages the dither away; without, it stays 0.  Not with --views or --ranks
//       --dof <focus_distance>:<blur_scale>[:<max_radius>]: the depth of field pass (include/svr_dof.h, HIP library only) with
//           --deferred 1: a thin-lens blur behind the fog pass (or the transparent objects), in front of --taa and --post;
//           blur_scale is the radius in pixels of a point at infinity, max_radius (default 16) the largest radius; the
//           pass as handed to the library is dumped as <prefix>.dof.  Not with --views or --ranks
//       --motion-blur <shutter>:<yaw_degrees>[:<max_blur>]: the camera motion blur pass (include/svr_motion.h, HIP library
//           only) with --deferred 1: streaks along the camera's motion behind --taa, in front of --auto-exposure and --post;
//           the previous frame's camera is this frame's turned by yaw_degrees, so one frame is deterministic; max_blur
//           (default 16) is the longest reach in pixels; the pass as handed to the library is dumped as <prefix>.motion.
//           Not with --views or --ranks
//       --taa <blend>: temporal antialiasing (include/svr_temporal.h, HIP library only): every frame is drawn with a sub-pixel
//           jitter (Halton(2, 3) - 0.5 pixels, a period of 16 frames) and resolved against the reprojected, clamped history
//           with the given weight of the current frame, behind the frame's last geometry or lighting pass and in front of
//           --post; not with --views or --ranks
//       --ao <radius>:<intensity>: screen-space ambient occlusion (include/svr_ambient.h, HIP library only) with --deferred 1:
//           svr_ambient_pass between the G-buffer pass and the lighting pass, which scales its ambient term by the result
//           (bias 0.02 radius, sharpness 0.05); an intensity of 0 gives the frame without the flag; not with --views or --ranks
//       --auto-exposure <key>:<adapt>: auto-exposure (include/svr_exposure.h, HIP library only) with --post: svr_meter_exposure
//           behind every frame's last pass and in front of the post pass, which multiplies --exposure (then a compensation)
//           by the metered exposure on the device; the final state is printed as
//           "exposure E target T mean_log2 M counted C black B meters N"
//       --stats-overlay 1: the UI overlay pass (include/svr_overlay.h, HIP library only): behind the last frame the colour
//           target is copied to a swapchain image in device memory and the reference's stats window (frametime, draw time,
//           update time, triangles, draws) is drawn onto it by svr_draw_overlay; <prefix>.swapchain is then that image and
//           <prefix>.overlay.txt the calls that built the list; not with --views or --ranks
//       --render-scale <s> [--upscale <sharpness>|off]: the reference's _render_scale (src/vk_engine.h:121), bound: --width and
//           --height are the window's; the frame is rendered at the reference's render extent (the float product truncated,
//           src/vk_engine.cpp:1220-1222) and <prefix>.color / .depth have that extent.  <prefix>.swapchain is the window-sized
//           image: with --upscale <sharpness 0..1> the upscaled present's (include/svr_upscale.h, HIP library only), with
//           --upscale off (the default) the scaled svr_copy_to_swapchain's, the reference's stretch.  --stats-overlay 1 draws
//           over either at the window's resolution.  s in (0, 1]; not with --views or --ranks
//       --occlusion off|last|prepass: occlusion culling (include/svr_occlusion.h, HIP library only): against the pyramid of
//           the previous frame's depth, or of a depth-only pass of the occluders (the opaque default material's objects;
//           with --gltf every opaque material's) drawn first; the dumps are those of --occlusion off
//       --select X,Y: after the last frame, print what won pixel (X, Y) (include/svr_ids.h, HIP library only):
//           select X Y object N mesh <name> surface S primitive P   or   select X Y none
//   svr_demo --lib libsvr_hip.so --dist libsvr_dist.so --ranks 2 [--transport shm|rccl] [--bounds 0,13,90] [--rebalance 1]
//       the sharded frame (include/svr_dist.h): one process per rank (forked before anything touches the GPU;
//       rccl: rank r on device r; shm: every rank on device 0), every rank dumps the exchanged image as
//       <prefix>.rank<r>.swapchain — it must be the single-process <prefix>.swapchain
//
// Scene: a three-level node hierarchy of cubes (exercises Node::refresh_transform's parent_matrix quirk and
// MeshNode::Draw's world*top order) with an opaque default material and a Transparent checker one.
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include <dlfcn.h>
#include <sys/wait.h>
#include <unistd.h>

#include "../../include/svr_dist.h"
#include "svr_engine.h"
#include "svr_image.h"

using namespace svrhost;

static void cube(std::vector<uint32_t>& idx, std::vector<SvrVertex>& vtx) {
  // 24 vertices / 36 indices, per-face uv in [0,1]^2, axial normals, colour 1 (same table as scenes.cube_mesh)
  const float faces[6][3][3] = {
      {{0, 0, 1}, {1, 0, 0}, {0, 1, 0}},  {{0, 0, -1}, {-1, 0, 0}, {0, 1, 0}}, {{1, 0, 0}, {0, 0, -1}, {0, 1, 0}},
      {{-1, 0, 0}, {0, 0, 1}, {0, 1, 0}}, {{0, 1, 0}, {1, 0, 0}, {0, 0, -1}},  {{0, -1, 0}, {1, 0, 0}, {0, 0, 1}}};
  const int corner[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
  for (int f = 0; f < 6; f++) {
    uint32_t base = (uint32_t)vtx.size();
    for (int c = 0; c < 4; c++) {
      SvrVertex v{};
      for (int k = 0; k < 3; k++) {
        v.position[k] = faces[f][0][k] * 0.5f + faces[f][1][k] * ((float)corner[c][0] - 0.5f) + faces[f][2][k] * ((float)corner[c][1] - 0.5f);
        v.normal[k] = faces[f][0][k];
      }
      v.uv_x = (float)corner[c][0];
      v.uv_y = (float)corner[c][1];
      v.color[0] = v.color[1] = v.color[2] = v.color[3] = 1.f;
      vtx.push_back(v);
    }
    const uint32_t q[6] = {0, 1, 2, 0, 2, 3};
    for (uint32_t i : q) idx.push_back(base + i);
  }
}

template <class T>
static void dump(const std::string& path, const T* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

static std::vector<pid_t> g_kids;  // rank 0 of --ranks N: the other ranks' processes
static bool g_exit_ok = false;

int main(int argc, char** argv) {
  std::string lib, prefix, gltf, png, dist_lib, transport = "shm", bounds_arg;
  int ranks = 1, rebalance = 0, queue_caps = 0, partition = 0, pick_partition = 0;
  uint32_t w = 160, h = 90;
  int frames = 2, background = 0, retained = 0;
  uint32_t views = 0;
  bool depth_only = false, deferred = false, stats_overlay = false;
  std::string occlusion = "off", post_arg, taa_arg, ao_arg, ae_arg, fog_arg, reflect_arg, dof_arg, motion_arg, scale_arg, upscale_arg = "off";
  SvrPostPass post{1.0f, 1.0f, 1.0f, 0, SVR_TONEMAP_CLAMP};
  float yaw = 0.f;
  bool set_yaw = false;
  bool select = false;
  uint32_t sel_x = 0, sel_y = 0;
  float cam[5] = {0, 0, 0, 0, 0};  // position, pitch, yaw
  uint32_t sw = 0, sh = 0;
  for (int i = 1; i + 1 < argc; i += 2) {
    std::string a = argv[i];
    if (a == "--lib") lib = argv[i + 1];
    else if (a == "--gltf") gltf = argv[i + 1];
    else if (a == "--dist") dist_lib = argv[i + 1];
    else if (a == "--ranks") ranks = atoi(argv[i + 1]);
    else if (a == "--transport") transport = argv[i + 1];
    else if (a == "--bounds") bounds_arg = argv[i + 1];
    else if (a == "--rebalance") rebalance = atoi(argv[i + 1]);
    else if (a == "--queue-caps") queue_caps = atoi(argv[i + 1]);   // SVR_OPT_QUEUE_CAPS: tiny queues, passes overflow and are replayed
    else if (a == "--partition") partition = std::string(argv[i + 1]) == "interleaved" ? 1 : 0;  // bands | interleaved
    else if (a == "--pick") pick_partition = atoi(argv[i + 1]);     // after N frames of each partition: keep the faster one
    else if (a == "--png") png = argv[i + 1];
    else if (a == "--background") background = atoi(argv[i + 1]);
    else if (a == "--retained") retained = atoi(argv[i + 1]);  // 1: draw through a draw list (include/svr_draw_list.h)
    else if (a == "--depth-only") depth_only = atoi(argv[i + 1]) != 0;  // depth-only passes (include/svr_depth.h)
    else if (a == "--deferred") deferred = atoi(argv[i + 1]) != 0;  // G-buffer pass, lighting pass, transparent objects under LOAD
    else if (a == "--post") post_arg = argv[i + 1];  // <operator>:<levels> (include/svr_post.h)
    else if (a == "--taa") taa_arg = argv[i + 1];  // <blend> (include/svr_temporal.h)
    else if (a == "--reflect") reflect_arg = argv[i + 1];  // <intensity>:<max_distance>[:<steps>] (include/svr_reflect.h)
    else if (a == "--fog") fog_arg = argv[i + 1];  // <density>:<falloff>[:<g>] (include/svr_fog.h)
    else if (a == "--dof") dof_arg = argv[i + 1];  // <focus_distance>:<blur_scale>[:<max_radius>] (include/svr_dof.h)
    else if (a == "--motion-blur") motion_arg = argv[i + 1];  // <shutter>:<yaw_degrees>[:<max_blur>] (include/svr_motion.h)
    else if (a == "--ao") ao_arg = argv[i + 1];  // <radius>:<intensity> (include/svr_ambient.h)
    else if (a == "--auto-exposure") ae_arg = argv[i + 1];  // <key>:<adapt> (include/svr_exposure.h)
    else if (a == "--stats-overlay") stats_overlay = atoi(argv[i + 1]) != 0;  // include/svr_overlay.h
    else if (a == "--render-scale") scale_arg = argv[i + 1];  // <s> (include/svr_upscale.h)
    else if (a == "--upscale") upscale_arg = argv[i + 1];  // <sharpness> | off
    else if (a == "--exposure") post.exposure = (float)atof(argv[i + 1]);
    else if (a == "--bloom-threshold") post.bloom_threshold = (float)atof(argv[i + 1]);
    else if (a == "--bloom-intensity") post.bloom_intensity = (float)atof(argv[i + 1]);
    else if (a == "--occlusion") occlusion = argv[i + 1];  // off | last | prepass (include/svr_occlusion.h)
    else if (a == "--views") views = (uint32_t)atoi(argv[i + 1]);  // N cameras in one multiview pass (include/svr_views.h)
    else if (a == "--yaw") { yaw = (float)atof(argv[i + 1]); set_yaw = true; }  // the camera's yaw (radians), after the scene's own
    else if (a == "--select" && sscanf(argv[i + 1], "%u,%u", &sel_x, &sel_y) == 2) select = true;  // (--pick is the partition pick)
    else if (a == "--swapchain" && sscanf(argv[i + 1], "%ux%u", &sw, &sh) == 2) {}
    else if (a == "--camera" && sscanf(argv[i + 1], "%f,%f,%f,%f,%f", &cam[0], &cam[1], &cam[2], &cam[3], &cam[4]) == 5) {}
    else if (a == "--width") w = (uint32_t)atoi(argv[i + 1]);
    else if (a == "--height") h = (uint32_t)atoi(argv[i + 1]);
    else if (a == "--frames") frames = atoi(argv[i + 1]);
    else if (a == "--dump") prefix = argv[i + 1];
  }
  if (!png.empty()) {  // decoder check: PNG file -> <prefix>.rgba (tests/test_gltf_loader.py)
    std::ifstream f(png, std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::string err;
    svrimg::Image img;
    const char* format = "";
    if (!svrimg::decode(bytes.data(), bytes.size(), img, &err, &format)) {
      fprintf(stderr, "%s: %s\n", format, err.c_str());
      return 1;
    }
    uint32_t iw = img.w, ih = img.h;
    std::vector<uint8_t> rgba;
    rgba.swap(img.rgba);
    printf("png %u %u %s\n", iw, ih, format);
    if (!prefix.empty()) dump(prefix + ".rgba", rgba.data(), rgba.size());
    return 0;
  }
  if (lib.empty()) {
    fprintf(stderr, "usage: svr_demo --lib <shared library exporting svr.h> [--width W --height H --frames N --dump prefix]\n"
                    "                [--gltf file.glb|file.gltf --camera x,y,z,pitch,yaw] [--background 0|1] [--swapchain WxH]\n"
                    "                [--retained 1] [--views N] [--yaw radians] [--depth-only 1] [--deferred 1]\n"
                    "                [--occlusion off|last|prepass]\n"
                    "                [--post clamp|reinhard|aces:<levels> --exposure E --bloom-threshold T --bloom-intensity I]\n"
                    "                [--taa blend] [--ao radius:intensity] [--auto-exposure key:adapt] [--stats-overlay 1]\n"
                    "                [--render-scale s --upscale sharpness|off] [--fog density:falloff[:g]]\n"
                    "                [--dof focus_distance:blur_scale[:max_radius]] [--motion-blur shutter:yaw_degrees[:max_blur]]\n"
                    "                [--reflect intensity:max_distance[:steps]]\n");
    return 2;
  }
  float taa_blend = 0.f;
  if (!taa_arg.empty()) {
    char* end = nullptr;
    taa_blend = strtof(taa_arg.c_str(), &end);
    if (!end || *end || end == taa_arg.c_str() || !(taa_blend > 0.f && taa_blend <= 1.f)) {
      fprintf(stderr, "--taa: expected a blend in (0, 1], got '%s'\n", taa_arg.c_str());
      return 2;
    }
    if (views) {
      fprintf(stderr, "--taa: not with --views (the pass works on the context's own colour target)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--taa: not with --ranks (a band rank would clamp taps at its band's edge and keep its own history)\n");
      return 1;
    }
  }
  float ao_radius = 0.f, ao_intensity = 0.f;
  if (!ao_arg.empty()) {
    const size_t colon = ao_arg.find(':');
    char *end_r = nullptr, *end_i = nullptr;
    ao_radius = strtof(ao_arg.c_str(), &end_r);
    if (colon != std::string::npos) ao_intensity = strtof(ao_arg.c_str() + colon + 1, &end_i);
    if (colon == std::string::npos || colon == 0 || end_r != ao_arg.c_str() + colon || !end_i || *end_i || end_i == ao_arg.c_str() + colon + 1 ||
        !(ao_radius > 0.f && ao_radius < INFINITY) || !(ao_intensity >= 0.f && ao_intensity < INFINITY)) {
      fprintf(stderr, "--ao: expected <radius > 0>:<intensity >= 0>, got '%s'\n", ao_arg.c_str());
      return 2;
    }
    if (!deferred) {
      fprintf(stderr, "--ao: needs --deferred 1 (the pass reads the G-buffer and the lighting pass applies it)\n");
      return 1;
    }
    if (views) {
      fprintf(stderr, "--ao: not with --views (the pass works on the context's own targets)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--ao: not with --ranks (a band rank would cut taps at its band's edge)\n");
      return 1;
    }
  }
  float reflect_intensity = 0.f, reflect_distance = 0.f;
  unsigned reflect_steps = 16;
  if (!reflect_arg.empty()) {
    char tail = 0;
    const int n = sscanf(reflect_arg.c_str(), "%f:%f:%u%c", &reflect_intensity, &reflect_distance, &reflect_steps, &tail);
    char tail2 = 0;
    const int n2 = n == 2 ? sscanf(reflect_arg.c_str(), "%f:%f%c", &reflect_intensity, &reflect_distance, &tail2) : 0;
    const bool shape = (n == 3 && reflect_arg.find('-', reflect_arg.rfind(':')) == std::string::npos) || (n == 2 && n2 == 2);
    if (!shape || !(reflect_intensity >= 0.f && reflect_intensity < INFINITY) || !(reflect_distance > 0.f && reflect_distance < INFINITY) ||
        reflect_steps < 1 || reflect_steps > SVR_REFLECT_MAX_STEPS) {
      fprintf(stderr, "--reflect: expected <intensity >= 0>:<max_distance > 0>[:<steps in 1..64>], got '%s'\n", reflect_arg.c_str());
      return 2;
    }
    if (!deferred) {
      fprintf(stderr, "--reflect: needs --deferred 1 (the pass runs behind the lighting pass and the transparent objects)\n");
      return 1;
    }
    if (views) {
      fprintf(stderr, "--reflect: not with --views (the pass works on the context's own targets)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--reflect: not with --ranks (a band rank would reflect what its own rows hold)\n");
      return 1;
    }
  }
  float fog_density = 0.f, fog_falloff = 0.f, fog_g = 0.f;
  if (!fog_arg.empty()) {
    char tail = 0;
    const int n = sscanf(fog_arg.c_str(), "%f:%f:%f%c", &fog_density, &fog_falloff, &fog_g, &tail);
    char tail2 = 0;
    const int n2 = n == 2 ? sscanf(fog_arg.c_str(), "%f:%f%c", &fog_density, &fog_falloff, &tail2) : 0;
    const bool shape = n == 3 || (n == 2 && n2 == 2);
    if (!shape || !(fog_density >= 0.f && fog_density < INFINITY) || !(fog_falloff >= 0.f && fog_falloff < INFINITY) || !(fog_g > -1.f && fog_g < 1.f)) {
      fprintf(stderr, "--fog: expected <density >= 0>:<falloff >= 0>[:<g in (-1, 1)>], got '%s'\n", fog_arg.c_str());
      return 2;
    }
    if (!deferred) {
      fprintf(stderr, "--fog: needs --deferred 1 (the pass runs behind the lighting pass and the transparent objects)\n");
      return 1;
    }
    if (views) {
      fprintf(stderr, "--fog: not with --views (the pass works on the context's own targets)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--fog: not with --ranks (a band rank would clamp the upsample's taps at its band's edge)\n");
      return 1;
    }
  }
  float dof_focus = 0.f, dof_scale = 0.f, dof_max = (float)SVR_DOF_MAX_RADIUS;
  if (!dof_arg.empty()) {
    char tail = 0;
    const int n = sscanf(dof_arg.c_str(), "%f:%f:%f%c", &dof_focus, &dof_scale, &dof_max, &tail);
    char tail2 = 0;
    const int n2 = n == 2 ? sscanf(dof_arg.c_str(), "%f:%f%c", &dof_focus, &dof_scale, &tail2) : 0;
    const bool shape = n == 3 || (n == 2 && n2 == 2);
    if (!shape || !(dof_focus > 0.f && dof_focus < INFINITY) || !(dof_scale >= 0.f && dof_scale < INFINITY) || !(dof_max >= 0.f && dof_max <= (float)SVR_DOF_MAX_RADIUS)) {
      fprintf(stderr, "--dof: expected <focus_distance > 0>:<blur_scale >= 0>[:<max_radius in 0..16>], got '%s'\n", dof_arg.c_str());
      return 2;
    }
    if (!deferred) {
      fprintf(stderr, "--dof: needs --deferred 1 (the pass runs behind the lighting pass and the transparent objects)\n");
      return 1;
    }
    if (views) {
      fprintf(stderr, "--dof: not with --views (the pass works on the context's own targets)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--dof: not with --ranks (a band rank would clamp its taps and cells at its band's edge)\n");
      return 1;
    }
  }
  float motion_shutter = 0.f, motion_yaw = 0.f, motion_max = (float)SVR_MOTION_MAX_BLUR;
  if (!motion_arg.empty()) {
    char tail = 0;
    const int n = sscanf(motion_arg.c_str(), "%f:%f:%f%c", &motion_shutter, &motion_yaw, &motion_max, &tail);
    char tail2 = 0;
    const int n2 = n == 2 ? sscanf(motion_arg.c_str(), "%f:%f%c", &motion_shutter, &motion_yaw, &tail2) : 0;
    const bool shape = n == 3 || (n == 2 && n2 == 2);
    if (!shape || !(motion_shutter >= 0.f && motion_shutter < INFINITY) || !(motion_yaw > -INFINITY && motion_yaw < INFINITY) ||
        !(motion_max >= 0.f && motion_max <= (float)SVR_MOTION_MAX_BLUR)) {
      fprintf(stderr, "--motion-blur: expected <shutter >= 0>:<yaw_degrees>[:<max_blur in 0..16>], got '%s'\n", motion_arg.c_str());
      return 2;
    }
    if (!deferred) {
      fprintf(stderr, "--motion-blur: needs --deferred 1 (the pass runs behind the lighting pass and the transparent objects)\n");
      return 1;
    }
    if (views) {
      fprintf(stderr, "--motion-blur: not with --views (the pass works on the context's own targets)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--motion-blur: not with --ranks (a band rank would clamp its taps and cells at its band's edge)\n");
      return 1;
    }
  }
  if (!post_arg.empty()) {
    const size_t colon = post_arg.find(':');
    const std::string op = post_arg.substr(0, colon);
    char* end = nullptr;
    const long levels = colon == std::string::npos ? -1 : strtol(post_arg.c_str() + colon + 1, &end, 10);
    const bool known = op == "clamp" || op == "reinhard" || op == "aces";
    post.tonemap = op == "aces" ? SVR_TONEMAP_ACES : (op == "reinhard" ? SVR_TONEMAP_REINHARD : SVR_TONEMAP_CLAMP);
    if (!known || levels < 0 || levels > SVR_POST_MAX_LEVELS || !end || *end || end == post_arg.c_str() + colon + 1) {
      fprintf(stderr, "--post: expected clamp|reinhard|aces:<levels 0..%d>, got '%s'\n", SVR_POST_MAX_LEVELS, post_arg.c_str());
      return 2;
    }
    post.bloom_levels = (uint32_t)levels;
    if (views) {
      fprintf(stderr, "--post: not with --views (the pass works on the context's own colour target)\n");
      return 1;
    }
    if (ranks > 1) {
      fprintf(stderr, "--post: not with --ranks (a band rank would bloom its own rows only)\n");
      return 1;
    }
  }
  float render_scale = 1.f, upscale_sharpness = 0.f;
  const bool upscale = upscale_arg != "off";
  if (!scale_arg.empty()) {
    char* end = nullptr;
    render_scale = strtof(scale_arg.c_str(), &end);
    if (!end || *end || end == scale_arg.c_str() || !(render_scale > 0.f && render_scale <= 1.f)) {
      fprintf(stderr, "--render-scale: expected a scale in (0, 1], got '%s'\n", scale_arg.c_str());
      return 2;
    }
    if (views || ranks > 1) {
      fprintf(stderr, "--render-scale: not with --views or --ranks\n");
      return 1;
    }
  }
  if (upscale) {
    char* end = nullptr;
    upscale_sharpness = strtof(upscale_arg.c_str(), &end);
    if (!end || *end || end == upscale_arg.c_str() || !(upscale_sharpness >= 0.f && upscale_sharpness <= 1.f)) {
      fprintf(stderr, "--upscale: expected a sharpness in [0, 1] or off, got '%s'\n", upscale_arg.c_str());
      return 2;
    }
    if (views || ranks > 1) {
      fprintf(stderr, "--upscale: not with --views or --ranks\n");
      return 1;
    }
  }
  if (stats_overlay && (views || ranks > 1)) {
    fprintf(stderr, "--stats-overlay: not with --views or --ranks\n");
    return 1;
  }
  float ae_key = 0.f, ae_adapt = 0.f;
  if (!ae_arg.empty()) {
    const size_t colon = ae_arg.find(':');
    char *end_k = nullptr, *end_a = nullptr;
    ae_key = strtof(ae_arg.c_str(), &end_k);
    if (colon != std::string::npos) ae_adapt = strtof(ae_arg.c_str() + colon + 1, &end_a);
    if (colon == std::string::npos || colon == 0 || end_k != ae_arg.c_str() + colon || !end_a || *end_a || end_a == ae_arg.c_str() + colon + 1 ||
        !(ae_key > 0.f && ae_key < INFINITY) || !(ae_adapt >= 0.f && ae_adapt <= 1.f)) {
      fprintf(stderr, "--auto-exposure: expected <key > 0>:<adapt 0..1>, got '%s'\n", ae_arg.c_str());
      return 2;
    }
    if (post_arg.empty()) {
      fprintf(stderr, "--auto-exposure: needs --post (the post pass is what applies the metered exposure)\n");
      return 1;
    }
  }
  // the sharded frame: one process per rank, forked before anything touches the GPU; rank 0 makes the id
  int rank = 0;
  std::vector<int> id_pipe_r(ranks > 1 ? ranks : 0, -1), id_pipe_w(ranks > 1 ? ranks : 0, -1);
  if (ranks > 1) {
    if (dist_lib.empty()) {
      fprintf(stderr, "--ranks needs --dist <libsvr_dist.so>\n");
      return 2;
    }
    for (int r = 1; r < ranks; r++) {
      int fd[2];
      if (pipe(fd) != 0) return 1;
      id_pipe_r[r] = fd[0];
      id_pipe_w[r] = fd[1];
    }
    std::vector<pid_t> kids;
    for (int r = 1; r < ranks; r++) {
      pid_t pid = fork();
      if (pid < 0) return 1;
      if (pid == 0) {
        rank = r;
        kids.clear();
        break;
      }
      kids.push_back(pid);
    }
    if (rank == 0 && !kids.empty()) {  // rank 0 is the parent itself; it reaps the others at the end (below)
      g_kids = kids;
      // a rank that fails must not leave the others waiting for it (a test would sit out its timeout): when a child
      // exits with an error the parent kills the rest and goes; when the parent itself fails, it takes the children along
      struct sigaction sa {};
      sa.sa_handler = [](int) {
        int st = 0;
        pid_t p;
        while ((p = waitpid(-1, &st, WNOHANG)) > 0) {
          for (pid_t& k : g_kids)
            if (k == p) k = -1;
          if (!(WIFEXITED(st) && WEXITSTATUS(st) == 0)) {
            for (pid_t k : g_kids)
              if (k > 0) kill(k, SIGKILL);
            _exit(3);
          }
        }
      };
      sa.sa_flags = SA_RESTART | SA_NOCLDSTOP;
      sigaction(SIGCHLD, &sa, nullptr);
      atexit([] {
        signal(SIGCHLD, SIG_DFL);
        for (pid_t p : g_kids) {
          if (p <= 0) continue;
          if (!g_exit_ok) kill(p, SIGKILL);
          int st = 0;
          waitpid(p, &st, 0);
        }
      });
    }
  }
  SvrEngine eng;
  eng.device = transport == "rccl" ? rank : 0;
  eng.render_scale = render_scale;
  eng.upscale = upscale;
  eng.upscale_sharpness = upscale_sharpness;
  if (!eng.init(lib, w, h)) {
    fprintf(stderr, "%s%s\n", eng.error.rfind("--", 0) == 0 ? "" : "init failed: ", eng.error.c_str());
    return 1;
  }
  printf("backend %s, %ux%u\n", eng.api.svr_backend_name(), w, h);
  if (!scale_arg.empty()) printf("render extent %ux%u\n", eng.width, eng.height);

  eng.current_background_effect = background;
  eng.retained = retained != 0;
  if (occlusion == "last") eng.occlusion = SvrEngine::Occlusion::Last;
  else if (occlusion == "prepass") eng.occlusion = SvrEngine::Occlusion::Prepass;
  else if (occlusion != "off") {
    fprintf(stderr, "--occlusion: off, last or prepass\n");
    return 2;
  }
  eng.swapchain_width = sw;
  eng.swapchain_height = sh;
  if (!gltf.empty()) {  // VulkanEngine::init: load_gltf_meshes(this, path) -> loaded_scenes["structure"] (src/vk_engine.cpp:192-198)
    auto loaded = load_gltf_meshes(&eng, gltf);
    if (!loaded) {
      fprintf(stderr, "%s\n", eng.error.c_str());
      return 1;
    }
    eng.loaded_scenes["structure"] = loaded;
    eng.main_camera.position = {cam[0], cam[1], cam[2]};
    eng.main_camera.pitch = cam[3];
    eng.main_camera.yaw = cam[4];
    size_t surfaces = 0;
    for (auto& m : loaded->meshes) surfaces += m->surfaces.size();
    printf("gltf %s: %zu meshes %zu surfaces %zu nodes %zu top nodes %zu materials %zu images %zu samplers\n", gltf.c_str(),
           loaded->meshes.size(), surfaces, loaded->nodes.size(), loaded->top_nodes.size(), loaded->materials.size(),
           loaded->images.size(), loaded->samplers.size());
    for (auto& m : loaded->materials)
      if (m->pass_type == SVR_PASS_MAIN_COLOR) eng.occluder_materials.push_back(m->handle);
  } else {
  // "load_gltf_meshes" by hand: one mesh with two primitives (two cubes' worth of geometry in one buffer)
  auto mesh = std::make_shared<MeshAsset>();
  mesh->name = "cubes";
  std::vector<uint32_t> idx;
  std::vector<SvrVertex> vtx;
  const float tint[4] = {0.4f, 0.3f, 0.2f, 1.f};
  auto transparent = eng.write_material(SVR_PASS_TRANSPARENT, tint, eng.error_checkerboard_image, eng.default_sampler_nearest);
  auto opaque = std::make_shared<MaterialInstance>(eng.default_data);
  eng.occluder_materials.push_back(opaque->handle);  // --occlusion prepass: the opaque cubes are the occluders
  for (int prim = 0; prim < 2; prim++) {
    size_t initial_vtx = vtx.size();
    std::vector<uint32_t> ci;
    std::vector<SvrVertex> cv;
    cube(ci, cv);
    for (auto& v : cv) v.position[0] += 1.25f * (float)prim;  // second primitive sits beside the first
    GeoSurface s;
    s.startIndex = (uint32_t)idx.size();
    s.count = (uint32_t)ci.size();
    for (uint32_t i : ci) idx.push_back(i + (uint32_t)initial_vtx);  // indices rebased, src/vk_loader.cpp:311-312
    vtx.insert(vtx.end(), cv.begin(), cv.end());
    s.bounds = loader_bounds(vtx, initial_vtx);
    s.material = prim == 0 ? opaque : transparent;
    mesh->surfaces.push_back(s);
  }
  mesh->meshBuffers = eng.upload_mesh(idx, vtx);

  auto scene = std::make_shared<LoadedScene>();
  scene->meshes.push_back(mesh);
  auto trs = [](svrm::vec3 t, svrm::quat q, svrm::vec3 s) {  // src/vk_loader.cpp:400-410: tm * rm * sm
    return svrm::mul(svrm::mul(svrm::translate(svrm::identity(), t), svrm::to_mat4(q)), svrm::scale(svrm::identity(), s));
  };
  auto root = std::make_shared<Node>();
  root->local_transform = trs({0, 0, -12}, {1, 0, 0, 0}, {1, 1, 1});
  auto child = std::make_shared<MeshNode>();
  child->mesh = mesh;
  child->local_transform = trs({-3, 0, -9}, {0.70710677f, 0, 0.70710677f, 0}, {2, 2, 2});
  auto grandchild = std::make_shared<MeshNode>();
  grandchild->mesh = mesh;
  grandchild->local_transform = trs({2, 1.5f, -7}, {1, 0, 0, 0}, {1, 1.5f, 1});
  root->children.push_back(child);
  child->parent = root;
  child->children.push_back(grandchild);
  grandchild->parent = child;
  scene->nodes = {root, child, grandchild};
  scene->top_nodes = {root};
  root->refresh_transform(svrm::identity());  // src/vk_loader.cpp:430-435
  eng.loaded_scenes["structure"] = scene;
  eng.main_camera.position = {0, 0, 0};
  }

  if (!dist_lib.empty()) {
    void* dh = dlopen(dist_lib.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!dh) {
      fprintf(stderr, "dlopen %s: %s\n", dist_lib.c_str(), dlerror());
      return 1;
    }
#define DIST_FN(name) auto name##_ = reinterpret_cast<decltype(&::name)>(dlsym(dh, #name)); if (!name##_) { fprintf(stderr, "missing %s\n", #name); return 1; }
    DIST_FN(svr_dist_get_unique_id) DIST_FN(svr_dist_create) DIST_FN(svr_dist_destroy) DIST_FN(svr_dist_set_bounds) DIST_FN(svr_dist_get_bounds)
    DIST_FN(svr_dist_rebalance) DIST_FN(svr_dist_band) DIST_FN(svr_dist_begin_frame) DIST_FN(svr_dist_end_frame) DIST_FN(svr_dist_wait_frame)
    DIST_FN(svr_dist_read_frame) DIST_FN(svr_dist_last_error) DIST_FN(svr_dist_set_partition) DIST_FN(svr_dist_get_partition) DIST_FN(svr_dist_pick_partition)
    DIST_FN(svr_dist_replays)
#undef DIST_FN
    const int tr = transport == "rccl" ? SVR_DIST_RCCL : SVR_DIST_SHM;
    uint8_t id[SVR_DIST_ID_BYTES];
    if (rank == 0) {
      if (svr_dist_get_unique_id_(tr, id) != SVR_OK) {
        fprintf(stderr, "unique id: %s\n", svr_dist_last_error_());
        return 1;
      }
      for (int r = 1; r < ranks; r++)
        if (write(id_pipe_w[r], id, sizeof(id)) != (ssize_t)sizeof(id)) return 1;
    } else if (read(id_pipe_r[rank], id, sizeof(id)) != (ssize_t)sizeof(id)) {
      return 1;
    }
    SvrDist* dist = nullptr;
    if (svr_dist_create_(eng.ctx, tr, id, rank, ranks, w, h, SVR_SWAPCHAIN_B8G8R8A8, &dist) != SVR_OK) {
      fprintf(stderr, "rank %d: svr_dist_create: %s\n", rank, svr_dist_last_error_());
      return 1;
    }
    if (!bounds_arg.empty()) {
      std::vector<uint32_t> b;
      for (size_t p = 0; p < bounds_arg.size();) {
        b.push_back((uint32_t)strtoul(bounds_arg.c_str() + p, nullptr, 10));
        size_t c = bounds_arg.find(',', p);
        p = c == std::string::npos ? bounds_arg.size() : c + 1;
      }
      if (svr_dist_set_bounds_(dist, b.data(), b.size()) != SVR_OK) {
        fprintf(stderr, "rank %d: svr_dist_set_bounds: %s\n", rank, svr_dist_last_error_());
        return 1;
      }
    }
    // (SVR_OPT_TUNING bit 4 with it: the overflow is found at a fence, not in passing, so the present behind the
    // void pass is void too and the exchange carries stale rows — the case svr_dist_wait_frame repairs)
    if (queue_caps > 0 && (eng.api.svr_set_option(eng.ctx, SVR_OPT_QUEUE_CAPS, queue_caps) != SVR_OK ||
                           eng.api.svr_set_option(eng.ctx, SVR_OPT_TUNING, 16) != SVR_OK)) {
      fprintf(stderr, "rank %d: SVR_OPT_QUEUE_CAPS: %s\n", rank, eng.api.svr_last_error());
      return 1;
    }
    if (svr_dist_set_partition_(dist, partition) != SVR_OK) return 1;
    int in_flight = 0;
    std::vector<uint8_t> image((size_t)w * h * 4);
    double pick_ms[2] = {0, 0};
    for (int f = 0; f < frames; f++) {
      if (pick_partition > 0 && f <= 2 * pick_partition && f % pick_partition == 0) {
        // --pick N: N frames in bands, N interleaved, each timed by this rank; then the collective choice.  The switch
        // happens between two frames on every rank alike.
        while (in_flight > 0) {
          if (svr_dist_wait_frame_(dist, nullptr) != SVR_OK) return 1;
          in_flight--;
        }
        eng.api.svr_sync(eng.ctx);
        SvrStats st{};
        eng.api.svr_get_stats(eng.ctx, &st);
        if (f > 0) pick_ms[f / pick_partition - 1] = st.gpu_time_ms;
        if (f == 2 * pick_partition) {
          int picked = -1;
          if (svr_dist_pick_partition_(dist, (float)pick_ms[0], (float)pick_ms[1], &picked) != SVR_OK) {
            fprintf(stderr, "rank %d: pick_partition: %s\n", rank, svr_dist_last_error_());
            return 1;
          }
          if (rank == 0) printf("frame %d: bands %.4f ms, interleaved %.4f ms on this rank -> %s\n", f, pick_ms[0], pick_ms[1], picked ? "interleaved" : "bands");
        } else {
          if (svr_dist_set_partition_(dist, f / pick_partition) != SVR_OK) return 1;
          eng.api.svr_set_option(eng.ctx, SVR_OPT_KERNEL_TIMING, 2);  // resets the running means
        }
      }
      if (rebalance && f > 0 && f % rebalance == 0) {  // a collective between two frames: every rank, same frame
        eng.api.svr_sync(eng.ctx);
        SvrStats st{};
        eng.api.svr_get_stats(eng.ctx, &st);
        int changed = 0;
        if (svr_dist_rebalance_(dist, st.tile_ms, &changed) != SVR_OK) {
          fprintf(stderr, "rank %d: rebalance: %s\n", rank, svr_dist_last_error_());
          return 1;
        }
        std::vector<uint32_t> b((size_t)ranks + 1);
        svr_dist_get_bounds_(dist, b.data(), b.size());
        if (rank == 0) {
          printf("frame %d: rows", f);
          for (uint32_t v : b) printf(" %u", v);
          printf("%s\n", changed ? " (re-cut)" : "");
        }
      }
      if (in_flight == 2) {  // both slots busy: take the older frame first (this is where present was)
        if (svr_dist_wait_frame_(dist, nullptr) != SVR_OK) return 1;
        in_flight--;
      }
      uint32_t y0 = 0, rows = 0;
      svr_dist_band_(dist, &y0, &rows);  // (interleaved: every rank draws; one without a tile row of its own draws nothing)
      if (svr_dist_begin_frame_(dist) != SVR_OK) {
        fprintf(stderr, "rank %d: begin_frame: %s\n", rank, svr_dist_last_error_());
        return 1;
      }
      eng.update_scene();
      int part_now = 0;
      svr_dist_get_partition_(dist, &part_now);
      if ((rows || part_now == SVR_DIST_INTERLEAVED) && (!eng.draw_background() || !eng.draw_geometry())) {
        fprintf(stderr, "rank %d: draw failed: %s\n", rank, eng.error.c_str());
        return 1;
      }
      if (svr_dist_end_frame_(dist) != SVR_OK) {
        fprintf(stderr, "rank %d: end_frame: %s\n", rank, svr_dist_last_error_());
        return 1;
      }
      in_flight++;
    }
    while (in_flight > 1) {
      if (svr_dist_wait_frame_(dist, nullptr) != SVR_OK) return 1;
      in_flight--;
    }
    if (svr_dist_read_frame_(dist, image.data(), image.size()) != SVR_OK) {
      fprintf(stderr, "rank %d: read_frame: %s\n", rank, svr_dist_last_error_());
      return 1;
    }
    if (!prefix.empty()) dump(prefix + ".rank" + std::to_string(rank) + ".swapchain", image.data(), image.size());
    uint32_t again = 0;
    svr_dist_replays_(dist, &again);
    SvrStats st{};
    eng.api.svr_get_stats(eng.ctx, &st);
    printf("rank %d of %d (%s): %d frames, last one exchanged; %u passes replayed, %u frames exchanged again\n", rank, ranks,
           transport.c_str(), frames, st.replayed_passes, again);
    svr_dist_destroy_(dist);
    eng.cleanup();
    g_exit_ok = true;
    return 0;
  }
  if (set_yaw) eng.main_camera.yaw = yaw;
  eng.views = views;
  if (depth_only && views) {
    fprintf(stderr, "--depth-only: not with --views\n");
    return 1;
  }
  if (eng.occlusion != SvrEngine::Occlusion::Off && views) {
    fprintf(stderr, "--occlusion: not with --views (multiview passes do not cull)\n");
    return 1;
  }
  if (deferred && (views || depth_only || retained || eng.occlusion != SvrEngine::Occlusion::Off)) {
    fprintf(stderr, "--deferred: not with --views, --depth-only, --retained or --occlusion\n");
    return 1;
  }
  if (!ae_arg.empty() && !(eng.api.svr_meter_exposure && eng.api.svr_set_post_auto_exposure && eng.api.svr_read_exposure)) {
    fprintf(stderr, "--auto-exposure: the library has no auto-exposure (include/svr_exposure.h)\n");
    return 1;
  }
  if (stats_overlay && !(eng.api.svr_draw_overlay && eng.api.svr_overlay_font)) {
    fprintf(stderr, "--stats-overlay: the library has no overlay pass (include/svr_overlay.h)\n");
    return 1;
  }
  if (!post_arg.empty() && !eng.api.svr_post_pass) {
    fprintf(stderr, "--post: the library has no post pass (include/svr_post.h)\n");
    return 1;
  }
  if (!reflect_arg.empty() && !eng.api.svr_reflect_pass) {
    fprintf(stderr, "--reflect: the library has no reflection pass (include/svr_reflect.h)\n");
    return 1;
  }
  if (!fog_arg.empty() && !eng.api.svr_fog_pass) {
    fprintf(stderr, "--fog: the library has no fog pass (include/svr_fog.h)\n");
    return 1;
  }
  if (!dof_arg.empty() && !eng.api.svr_dof_pass) {
    fprintf(stderr, "--dof: the library has no depth of field pass (include/svr_dof.h)\n");
    return 1;
  }
  if (!motion_arg.empty() && !eng.api.svr_motion_blur_pass) {
    fprintf(stderr, "--motion-blur: the library has no motion blur pass (include/svr_motion.h)\n");
    return 1;
  }
  if (!taa_arg.empty() && !eng.api.svr_temporal_resolve) {
    fprintf(stderr, "--taa: the library has no temporal pass (include/svr_temporal.h)\n");
    return 1;
  }
  if (!ao_arg.empty() && !eng.api.svr_ambient_pass) {
    fprintf(stderr, "--ao: the library has no ambient pass (include/svr_ambient.h)\n");
    return 1;
  }
  eng.taa_blend = taa_blend;
  eng.ao_radius = ao_radius;
  eng.ao_intensity = ao_intensity;
  if (select && !eng.enable_ids()) {
    fprintf(stderr, "--select: %s\n", eng.error.c_str());
    return 1;
  }
  for (int f = 0; f < frames; f++) {
    eng.update_scene();
    if (f == frames - 1 && !prefix.empty()) {
      dump(prefix + ".scene", &eng.scene_data, 1);
      dump(prefix + ".opaque", eng.main_draw_context.opaque_surfaces.data(), eng.main_draw_context.opaque_surfaces.size());
      dump(prefix + ".transparent", eng.main_draw_context.transparent_surfaces.data(), eng.main_draw_context.transparent_surfaces.size());
    }
    if (!eng.draw_background() || !(views ? eng.draw_geometry_views() : (depth_only ? eng.draw_depth() : (deferred ? eng.draw_deferred() : eng.draw_geometry())))) {
      fprintf(stderr, "draw failed: %s\n", eng.error.c_str());
      return 1;
    }
    // behind the lighting pass and the deferred frame's transparents, in front of the fog pass: the medium also lies between the
    // camera and a reflection
    if (!reflect_arg.empty() && !eng.reflect_pass(reflect_intensity, reflect_distance, reflect_steps, taa_blend > 0.f ? (uint32_t)f : 0u)) {
      fprintf(stderr, "%s\n", eng.error.rfind("--reflect", 0) == 0 ? eng.error.c_str() : ("--reflect: " + eng.error).c_str());
      return 1;
    }
    // behind the deferred frame's transparents, in front of the resolve (which averages the per-frame dither) and the post pass
    if (!fog_arg.empty() && !eng.fog_pass(fog_density, fog_falloff, fog_g, taa_blend > 0.f ? (uint32_t)f : 0u)) {
      fprintf(stderr, "%s\n", eng.error.rfind("--fog", 0) == 0 ? eng.error.c_str() : ("--fog: " + eng.error).c_str());
      return 1;
    }
    // behind the fog pass, in front of the resolve and the post pass: on scene-linear values, so that bloom sees the bokeh
    if (!dof_arg.empty() && !eng.dof_pass(dof_focus, dof_scale, dof_max)) {
      fprintf(stderr, "%s\n", eng.error.rfind("--dof", 0) == 0 ? eng.error.c_str() : ("--dof: " + eng.error).c_str());
      return 1;
    }
    if (taa_blend > 0.f && !eng.temporal_resolve()) {  // behind the frame's last pass, in front of the post pass
      fprintf(stderr, "%s\n", eng.error.rfind("--taa", 0) == 0 ? eng.error.c_str() : ("--taa: " + eng.error).c_str());
      return 1;
    }
    // behind the resolve, so that the history stays sharp; in front of the meter and the post pass, so that bloom sees the streaks
    if (!motion_arg.empty() && !eng.motion_blur_pass(motion_shutter, motion_yaw, motion_max)) {
      fprintf(stderr, "%s\n", eng.error.rfind("--motion-blur", 0) == 0 ? eng.error.c_str() : ("--motion-blur: " + eng.error).c_str());
      return 1;
    }
    if (!ae_arg.empty() && !eng.meter_exposure(ae_key, ae_adapt)) {  // behind the frame's last pass, in front of the post pass
      fprintf(stderr, "%s\n", eng.error.rfind("--auto-exposure", 0) == 0 ? eng.error.c_str() : ("--auto-exposure: " + eng.error).c_str());
      return 1;
    }
    if (!post_arg.empty() && !eng.post_pass(post)) {  // behind the frame's last pass, before the swapchain copy
      fprintf(stderr, "%s\n", eng.error.rfind("--post", 0) == 0 ? eng.error.c_str() : ("--post: " + eng.error).c_str());
      return 1;
    }
  }
  eng.api.svr_sync(eng.ctx);
  printf("draws %d triangles %d update %.3f ms record %.3f ms\n", eng.stats.drawcall_count, eng.stats.triangle_count,
         eng.stats.scene_update_time, eng.stats.mesh_draw_time);
  if (!ae_arg.empty()) {
    SvrExposureState st{};
    if (!eng.read_exposure(st)) {
      fprintf(stderr, "%s\n", eng.error.c_str());
      return 1;
    }
    printf("exposure %.9g target %.9g mean_log2 %.9g counted %u black %u meters %u\n", (double)st.exposure, (double)st.target, (double)st.mean_log2,
           st.counted, st.black, st.meters);
  }
  if (select) {
    SvrEngine::Pick p;
    if (!eng.pick(sel_x, sel_y, p)) {
      fprintf(stderr, "--select: %s\n", eng.error.c_str());
      return 1;
    }
    if (p.hit)
      printf("select %u %u object %u mesh %s surface %u primitive %u\n", sel_x, sel_y, p.object, p.mesh.c_str(), p.surface, p.primitive);
    else
      printf("select %u %u none\n", sel_x, sel_y);
  }
  if (!prefix.empty()) {
    std::vector<uint16_t> color;
    std::vector<float> depth;
    if (!eng.read_color_rgba16f(color) || !eng.read_depth(depth)) {
      fprintf(stderr, "readback failed: %s\n", eng.error.c_str());
      return 1;
    }
    dump(prefix + ".color", color.data(), color.size());
    dump(prefix + ".depth", depth.data(), depth.size());
    if (!reflect_arg.empty()) {
      std::vector<float> normal, albedo;
      if (!eng.read_attribute(SVR_ATTR_NORMAL, normal) || !eng.read_attribute(SVR_ATTR_ALBEDO, albedo)) {
        fprintf(stderr, "readback failed: %s\n", eng.error.c_str());
        return 1;
      }
      dump(prefix + ".reflect", &eng.last_reflect, 1);
      dump(prefix + ".normal", normal.data(), normal.size());
      dump(prefix + ".albedo", albedo.data(), albedo.size());
    }
    if (!fog_arg.empty()) dump(prefix + ".fog", &eng.last_fog, 1);
    if (!dof_arg.empty()) dump(prefix + ".dof", &eng.last_dof, 1);
    if (!motion_arg.empty()) dump(prefix + ".motion", &eng.last_motion, 1);
    std::vector<uint8_t> swap;  // what copy_image leaves in the swapchain image (src/vk_engine.cpp:1277)
    std::string drawn;  // --stats-overlay: ... and what draw_imgui then draws onto it (src/vk_engine.cpp:1282)
    if (!(stats_overlay ? eng.stats_overlay(swap, drawn) : eng.read_swapchain(swap))) {
      fprintf(stderr, "swapchain readback failed: %s\n", eng.error.c_str());
      return 1;
    }
    dump(prefix + ".swapchain", swap.data(), swap.size());
    if (stats_overlay) dump(prefix + ".overlay.txt", drawn.data(), drawn.size());
  }
  if (views) {  // --views: layer k is what a run with --yaw <view k's yaw> leaves in the colour and depth targets
    std::vector<uint16_t> color;
    std::vector<float> depth;
    if (!eng.read_view_layers(color, depth)) {
      fprintf(stderr, "readback failed: %s\n", eng.error.c_str());
      return 1;
    }
    const size_t px = (size_t)w * h;
    for (uint32_t k = 0; k < views; k++) {
      printf("view %u yaw %.9g\n", k, (double)eng.view_yaw(k));
      if (!prefix.empty()) {
        dump(prefix + ".view" + std::to_string(k) + ".color", color.data() + px * 4 * k, px * 4);
        dump(prefix + ".view" + std::to_string(k) + ".depth", depth.data() + px * k, px);
      }
    }
  }
  eng.cleanup();
  return 0;
}
