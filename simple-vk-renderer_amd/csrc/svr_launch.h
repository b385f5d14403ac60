// svr_launch.h — host-callable launchers of the HIP kernels (one per kernel file).
#pragma once
#include <cstddef>

#include "../../include/svr_ambient.h"
#include "../../include/svr_dof.h"
#include "../../include/svr_exposure.h"
#include "../../include/svr_fog.h"
#include "../../include/svr_lighting.h"
#include "../../include/svr_motion.h"
#include "../../include/svr_overlay.h"
#include "../../include/svr_post.h"
#include "../../include/svr_reflect.h"
#include "../../include/svr_temporal.h"
#include "../../include/svr_upscale.h"
#include "svr_device.h"

namespace svr {

// k_geometry.hip
// copy_bytes / zero_bytes are rounded up to 16: both buffers must be padded accordingly
// n_draws: DrawDesc records at the head of the copy whose mvp the kernel fills in (viewproj * mat)
void launch_prologue(const void* host_src, void* dst, size_t copy_bytes, void* zero, size_t zero_bytes, uint32_t n_draws,
                     const SvrSceneData& scene, hipStream_t s);
// depth_only: a depth-only pass (include/svr_depth.h): the setup_kernel instances that store what phase A reads
void launch_setup(const FrameParams& P, bool depth_only, hipStream_t s);
void launch_mesh_vert(const SvrVertex* vtx, uint32_t first, uint32_t n, const float* world16,
                      const float* viewproj16, const float* color_factors4, float* out_clip,
                      float* out_varyings, hipStream_t s);
// vtx == nullptr: colored_triangle.vert (index only); else colored_triangle_mesh.vert with matrix16 (device memory)
void launch_vertex_shader(const SvrVertex* vtx, uint32_t first, uint32_t n, const float* matrix16, float* out_clip,
                          float* out_varyings, hipStream_t s);
// k_flatten.hip
void launch_flatten(const FlattenParams& F, hipStream_t s);
// a resident draw list (objects in device memory, in draw order): list_kernel up to LIST_FUSED_MAX objects, else the
// four kernels of launch_flatten (which then need F.objects_dev / keys / draw_tris / chunk_base scratch)
void launch_list_flatten(const FlattenParams& F, hipStream_t s);
// k_bin.hip
void launch_bin_count(const FrameParams& P, hipStream_t s);
void launch_bin_scan(const FrameParams& P, hipStream_t s);
void launch_bin_fill(const FrameParams& P, hipStream_t s, hipEvent_t done);  // done: signalled with the kernel (may be null)
// k_tile.hip
// depth_only: a depth-only pass (include/svr_depth.h): the tile_depth_kernel instances, which touch no colour
void launch_tiles(const FrameParams& P, int color_format, bool count_fragments, bool depth_only, hipStream_t s, hipEvent_t done);
// k_image.hip
// packed_pixel: the already encoded texel (RGBA16F: 4 halves, RGBA8: low 32 bits)
// poison: the context's sticky overflow flag (the clear is void while it is raised)
void launch_fill_color(void* color, uint32_t n_pixels, int color_format, uint64_t packed_pixel, const uint32_t* poison,
                       hipStream_t s);
void launch_background(void* color, int color_format, uint32_t W, uint32_t H, uint32_t y_first, uint32_t n_rows, int effect,
                       const float data[16], const uint32_t* poison, hipStream_t s);
// rstride / roff / row_end: the interleaved tile rows of svr_set_row_interleave (1, 0, row_first + n_rows: all rows);
// status: device word that receives 1 when the blit was void (poison), else status_ok (may be null)
void launch_blit(const void* color, int color_format, uint32_t W, uint32_t H, void* dst, uint32_t dw, uint32_t dh, uint32_t row_first,
                 uint32_t n_rows, int dst_format, const uint32_t* poison, uint32_t rstride, uint32_t roff, uint32_t row_end, uint32_t* status,
                 uint32_t status_ok, hipStream_t s);
// texel arena levels are tiled (svr_device.h texel_offset): splw, dplw, plw = log2 of a level's padded width (level_lw)
void launch_downsample(const uint8_t* src, uint32_t sw, uint32_t sh, uint32_t splw, uint8_t* dst, uint32_t dw, uint32_t dh,
                       uint32_t dplw, hipStream_t s);
void launch_retile(bool to_tiled, void* linear, uint8_t* tiled, uint32_t w, uint32_t h, uint32_t plw, hipStream_t s);
void launch_rgba16f_to_rgba8(const void* src, void* dst, uint32_t n_pixels, hipStream_t s);
// k_pyramid.hip: the depth pyramid of occlusion culling (include/svr_occlusion.h)
uint32_t pyramid_levels(uint32_t W, uint32_t H);
size_t pyramid_offsets(uint32_t W, uint32_t H, uint32_t* off);  // off[1 .. levels]: word offset of each level; returns the words
void launch_pyramid(const float* depth, uint32_t W, uint32_t H, uint32_t* pyr, const uint32_t* off, uint32_t n_levels,
                    const uint32_t* poison, hipStream_t s);
// the shadow map of a pass that takes one (C18; the lookup: svr_screen_math.h shadow_occluded)
struct ShadowMap {
  const float* depth;           // null: unshadowed, and nothing below is read
  uint32_t w, h;
  float half_w, half_h;         // Ws / 2, Hs / 2 (exact)
  float viewproj[16];
  float bias;
};
static_assert(sizeof(ShadowMap) == 96, "kernel arguments: the layout is part of the machine code");
// k_light.hip: the deferred lighting pass (include/svr_lighting.h)
struct LightLaunch {
  void* color;                  // the colour target (W x H), written where the albedo texel names an opaque winner
  const float* depth;           // W x H
  const float4* normal;         // the SVR_ATTR_NORMAL plane
  const float4* albedo;         // the SVR_ATTR_ALBEDO plane
  uint32_t W, H;
  uint32_t sx, sy, sw, sh;      // the scissor
  uint32_t tiles_x, rstride, roff;  // tile (x, y) of the grid is tile row y * rstride + roff of the scissor
  float two_over_w, two_over_h; // C17: 2.0f / float(W), 2.0f / float(H), divided on the host
  float inv_viewproj[16];
  float ambient_color[4], sunlight_direction[4], sunlight_color[4];
  const SvrPointLight* lights;  // device copy
  uint32_t n_lights;
  ShadowMap shadow;
  uint32_t* tile_counts;        // [tiles_x * tiles_y]: the lights each tile kept (svr_debug_read_light_tiles)
  const uint32_t* poison;
  const float* ao;              // the ambient target (include/svr_ambient.h), or null: light_kernel<FMT, true> / <FMT, false>
};
static_assert(sizeof(LightLaunch) == 328 && offsetof(LightLaunch, shadow) == 208, "where the flat shadow fields stood");
void launch_light(const LightLaunch& L, int color_format, uint32_t tiles_y, hipStream_t s);
// k_post.hip: the HDR post pass (include/svr_post.h)
struct PostLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  uint2* levels;                // the context's level images (B_i, then U_i in place): 4 halves per texel
  uint32_t n_levels;            // 0 .. SVR_POST_MAX_LEVELS
  uint32_t off[SVR_POST_MAX_LEVELS], lw[SVR_POST_MAX_LEVELS], lh[SVR_POST_MAX_LEVELS];  // C22: texel offset (even) and extent of each level
  float exposure, threshold, intensity;
  uint32_t tonemap;             // SVR_TONEMAP_*
  const uint32_t* poison;
  const float* auto_exposure;   // svr_set_post_auto_exposure: the state's exposure (include/svr_exposure.h), null when off
};
// C22: the level extents of a sw x sh image and their packed offsets (each level starts on 16 bytes); returns the texels
size_t post_level_layout(uint32_t sw, uint32_t sh, uint32_t n_levels, uint32_t* off, uint32_t* lw, uint32_t* lh);
// n_levels bloom_level_kernel launches, n_levels - 1 bloom_up_kernel launches and one post_composite_kernel, all on s
void launch_post(const PostLaunch& P, hipStream_t s);
// k_temporal.hip: temporal antialiasing (include/svr_temporal.h)
struct TemporalLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  const float* depth;           // the depth target, read as it stands in stream order
  uint32_t W, H;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  const uint2* hist_in;         // the history this resolve reads (W x H texels of 4 halves); read only where history_valid
  uint2* hist_out;              // ... and the one it writes: the roles are fixed at the call
  uint32_t history_valid;       // decided at the call (include/svr_temporal.h "History")
  uint32_t clamp;               // 0 under SVR_TEMPORAL_NO_CLAMP
  float reproject[16];
  float blend;
  float two_over_w, two_over_h; // C17: divided once, on the host
  float half_w, half_h;         // C29: W / 2, H / 2
  const uint32_t* poison;
};
// one temporal_resolve_kernel and one temporal_copy_kernel, on s
void launch_temporal(const TemporalLaunch& A, hipStream_t s);
// k_ambient.hip: screen-space ambient occlusion (include/svr_ambient.h)
struct AmbientLaunch {
  const float* depth;           // the depth target, read as it stands in stream order
  const float4* normal;         // the SVR_ATTR_NORMAL plane
  float2* raw;                  // the context's (a, 1/w) scratch plane (C36), W texels per row
  float* out;                   // the ambient target, W floats per row
  uint32_t W, H;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  float inv_viewproj[16];
  float two_over_w, two_over_h; // C17: divided once, on the host
  float radius_px;              // C33: radius * pixels_per_unit
  float radius2;                // C35: radius * radius
  float bias;
  float coef;                   // C36: (intensity * radius) * 0.125f
  float sharpness;
  uint32_t blur;                // 0 under SVR_AMBIENT_NO_BLUR
  const uint32_t* poison;
};
// one ambient_raw_kernel and one ambient_blur_kernel, on s
void launch_ambient(const AmbientLaunch& A, hipStream_t s);
// k_exposure.hip: auto-exposure (include/svr_exposure.h)
constexpr uint32_t EXPOSURE_STATE_WORDS = 8;   // SvrExposureState (6 words), padded to 32 bytes
constexpr uint32_t EXPOSURE_BINS_WORDS = 264;  // the working bins: SVR_EXPOSURE_BINS, then the black counter, padded
constexpr uint32_t EXPOSURE_WORDS = EXPOSURE_STATE_WORDS + EXPOSURE_BINS_WORDS + SVR_EXPOSURE_BINS;  // ... then the last histogram
struct ExposureLaunch {
  const uint2* color;           // the RGBA16F colour target, W texels per row: read only
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the pixels metered
  uint32_t* mem;                // the context's EXPOSURE_WORDS words: state, working bins (all 0 between meters), last histogram
  SvrExposureMeter meter;
  uint32_t snap;                // decided at the call (include/svr_exposure.h)
  const uint32_t* poison;
};
// C38's grid rule: the workgroups of exposure_histogram_kernel for a scissor of sw x sh
uint32_t exposure_grid(uint32_t sw, uint32_t sh);
// one exposure_histogram_kernel (none for an empty scissor) and one exposure_resolve_kernel, on s
void launch_exposure(const ExposureLaunch& A, hipStream_t s);
// k_overlay.hip: the UI overlay pass (include/svr_overlay.h)
constexpr uint32_t OVERLAY_REC_WORDS = 36;  // a triangle's record (k_overlay.hip "the record"), 144 bytes
// a command as the kernels read it: the clip box in whole pixels (C45), already cut to the image, and where its
// triangles stand among those of the launch
struct OverlayCmdDev {
  int32_t x0, y0, x1, y1;  // pixel i passes iff x0 <= i < x1
  uint32_t texture, vtx_offset, idx_offset;
  uint32_t tri_first, tri_count;  // among the triangles of the commands that reached the device, in order
  uint32_t pad[3];
};
static_assert(sizeof(OverlayCmdDev) == 48, "16-byte records");
struct OverlayLaunch {
  uint32_t* dst;                     // dw x dh UNORM8 texels, the caller's
  uint32_t dw, dh;
  int dst_fmt;                       // SVR_SWAPCHAIN_*
  float display_pos[2], scale[2];
  const SvrOverlayVertex* vertices;  // the context's device copies, valid for this launch
  const uint16_t* indices;
  const OverlayCmdDev* cmds;
  const SvrOverlayTexture* textures;
  uint32_t n_cmds, n_tris;           // commands and triangles that reached the device (n_tris > 0)
  uint32_t n_textures;               // entries of the texture table (<= SVR_OVERLAY_MAX_TEXTURES)
  uint32_t tile_x0, tile_y0, tiles_w, tiles_h;  // the 32 x 32 tiles the commands' clip boxes reach: the tile kernel's grid
  uint2* boxes;                      // [n_tris] the records' boxes alone, for the tile kernel's scan
  uint32_t* recs;                    // [n_tris][OVERLAY_REC_WORDS]
  uint32_t* stats;                   // SvrOverlayStats, written {submitted, 0, 0} by the copy in front of the kernels
  const uint32_t* poison;
};
// one overlay_setup_kernel and one overlay_tile_kernel, on s
void launch_overlay(const OverlayLaunch& A, hipStream_t s);
// k_upscale.hip: the upscaled present (include/svr_upscale.h)
struct UpscaleLaunch {
  const void* src;              // the colour target, W x H texels of src_fmt: read only
  int src_fmt;                  // SVR_COLOR_*
  uint32_t W, H;
  uint32_t* dst;                // dw x dh UNORM8 texels, the caller's (W <= dw, H <= dh)
  uint32_t dw, dh;
  int dst_fmt;                  // SVR_SWAPCHAIN_*
  float su, sv;                 // C51: (float)W / (float)dw and (float)H / (float)dh, divided once, on the host
  float peak;                   // C53: -1.0f / (8.0f - 3.0f * sharpness), computed once, at the call
  uint32_t sharpen;             // 0 under SVR_UPSCALE_NO_SHARPEN
  const uint32_t* poison;
  uint32_t* status;             // svr_set_present_status (may be null): 1 when void, else status_ok
};
// one upscale_kernel, on s
void launch_upscale(const UpscaleLaunch& A, uint32_t status_ok, hipStream_t s);
// k_fog.hip: the fog pass (include/svr_fog.h)
struct FogLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  const float* depth;           // the depth target, read as it stands in stream order
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  uint32_t gw, gh;              // C55: the half-resolution grid, (sw + 1) / 2 by (sh + 1) / 2
  float4* st;                   // the context's scratch: (S.rgb, T) per block, gw per row
  float* te;                    // ... and t_end per block
  float two_over_w, two_over_h; // C17: divided once, on the host
  float inv_viewproj[16];
  float cam[3];
  float density;
  float kh;                     // C57: height_falloff * log2(e), one product at the call
  float height_base, max_distance;
  uint32_t steps;
  float fog_color[3], sun_color[3];
  float sun[3];                 // C58: L / |L| (zero for a direction without a length)
  float one_plus_g2, minus_2g, one_minus_g2;  // C58: 1 + g g, -2 g, 1 - g g, computed once, at the call
  ShadowMap shadow;
  float edge;                   // C59: edge_sharpness
  uint32_t frame;
  const uint32_t* poison;
};
// C55: the blocks a context of W x H needs scratch for
inline size_t fog_blocks(uint32_t w, uint32_t h) { return (size_t)((w + 1u) / 2u) * ((h + 1u) / 2u); }
// one fog_march_kernel and one fog_composite_kernel, on s
void launch_fog(const FogLaunch& A, hipStream_t s);
// k_dof.hip: the depth of field pass (include/svr_dof.h)
struct DofLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  const float* depth;           // the depth target, read as it stands in stream order
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  uint32_t pitch;               // C62: texels per row of the prepared image, sw rounded up to even
  uint32_t cw, ch;              // C63: the cells, (sw + 7) / 8 by (sh + 7) / 8
  uint2* prep;                  // the context's scratch: the prepared image (san(rgb) and c, four halves per texel)
  float* cells;                 // ... and M per cell, cw per row
  float inv_z_scale, inv_z_bias;
  float neg_focus;              // C61: -focus_distance
  float blur_scale;
  float max_radius, neg_max_radius;
  uint32_t Rc;                  // C63: (ceil(max_radius) + 7) / 8
  const uint32_t* poison;
};
// C62, C63: the texels and the cells a context of W x H needs scratch for
inline size_t dof_texels(uint32_t w, uint32_t h) { return (size_t)((w + 1u) & ~1u) * h; }
inline size_t dof_cells(uint32_t w, uint32_t h) { return (size_t)((w + 7u) / 8u) * ((h + 7u) / 8u); }
// one dof_prepare_kernel and one dof_gather_kernel, on s
void launch_dof(const DofLaunch& A, hipStream_t s);
// k_motion.hip: the camera motion blur pass (include/svr_motion.h)
struct MotionLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  const float* depth;           // the depth target, read as it stands in stream order
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  uint32_t cw, ch;              // C69: the cells, (sw + 7) / 8 by (sh + 7) / 8
  uint4* prep;                  // the context's scratch: the prepared image (C68: san(rgb), the velocity halves, the depth's bits), sw per row
  unsigned long long* cells;    // ... and M per cell, cw per row
  float reproject[16];          // C67
  float two_over_w, two_over_h; // C17: divided once, on the host
  float half_w, half_h;         // C29: W / 2, H / 2
  float half_shutter;           // C67: 0.5 * shutter
  float max_blur;
  uint32_t Rc;                  // C69: (ceil(max_blur) + 7) / 8
  const uint32_t* poison;
};
// C68, C69: the texels and the cells a context of W x H needs scratch for
inline size_t motion_texels(uint32_t w, uint32_t h) { return (size_t)w * h; }
inline size_t motion_cells(uint32_t w, uint32_t h) { return (size_t)((w + 7u) / 8u) * ((h + 7u) / 8u); }
// one motion_prepare_kernel and one motion_gather_kernel, on s
void launch_motion(const MotionLaunch& A, hipStream_t s);
// k_reflect.hip: the reflection pass (include/svr_reflect.h)
struct ReflectLaunch {
  uint2* color;                 // the RGBA16F colour target, W texels per row: the scissor's RGB halves are rewritten in place
  const float* depth;           // the depth target, read as it stands in stream order
  const float4* normal;         // the SVR_ATTR_NORMAL plane
  const float4* albedo;         // the SVR_ATTR_ALBEDO plane: w says whether an opaque winner wrote the texel (C73)
  uint32_t W;
  uint32_t sx, sy, sw, sh;      // the scissor: the image of the pass
  uint32_t cw, ch;              // the trace's cells, (sw + 7) / 8 by (sh + 7) / 8
  float4* trace;                // the context's scratch: the trace texels (C77), sw per row
  uint32_t* cells;              // ... and per cell, cw per row: whether any of its trace texels is not 0
  float two_over_w, two_over_h; // C17: divided once, on the host
  float half_w, half_h;         // C75: W / 2, H / 2
  float x_lo, x_hi, y_lo, y_hi; // C75: the scissor as floats, sx <= fx < sx + sw (exact: the extents are below 2^24)
  float viewproj[16], inv_viewproj[16];
  float cam[3];
  float inv_z_scale, inv_z_bias;
  float delta;                  // C75: max_distance / steps, one quotient at the call
  float rmax;                   // C77: 1 / max_distance, likewise
  uint32_t steps, refine;
  float q_max;                  // C75: 1 + thickness, one sum at the call
  float f0, one_minus_f0;       // C77
  float intensity, distance_fade;
  float inv_edge;               // C77: 1 / edge_width; 0: no edge fade
  uint32_t resolve;
  float depth_tolerance;
  uint32_t frame;
  const uint32_t* poison;
};
// C77: the texels and the cells a context of W x H needs scratch for
inline size_t reflect_texels(uint32_t w, uint32_t h) { return (size_t)w * h; }
inline size_t reflect_cells(uint32_t w, uint32_t h) { return (size_t)((w + 7u) / 8u) * ((h + 7u) / 8u); }
// one reflect_trace_kernel and one reflect_resolve_kernel, on s
void launch_reflect(const ReflectLaunch& A, hipStream_t s);
void launch_rcp_sweep(int variant, unsigned long long first, unsigned long long count, unsigned long long* out19, hipStream_t s);

}  // namespace svr
