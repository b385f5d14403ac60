"""ctypes mirror of include/svr.h and a thin object wrapper over one loaded library.

The same binding drives the product (libsvr_hip.so) and, in tests only, the CPU oracle's library:
both export the identical C ABI.  Nothing here picks a library by itself; the product is loaded by
__init__.load_product_library(), the oracle only by the helpers under tests/.
"""
import ctypes as C
import os

import numpy as np


class SvrVertex(C.Structure):  # src/vk_types.h:97-103
    _fields_ = [("position", C.c_float * 3), ("uv_x", C.c_float), ("normal", C.c_float * 3),
                ("uv_y", C.c_float), ("color", C.c_float * 4)]


class SvrSceneData(C.Structure):  # src/vk_types.h:118-125
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("viewproj", C.c_float * 16),
                ("ambient_color", C.c_float * 4), ("sunlight_direction", C.c_float * 4),
                ("sunlight_color", C.c_float * 4)]


class SvrBounds(C.Structure):  # src/vk_loader.h:11-15
    _fields_ = [("origin", C.c_float * 3), ("sphere_radius", C.c_float), ("extents", C.c_float * 3)]


class SvrRenderObject(C.Structure):  # src/vk_engine.h:29-38
    _fields_ = [("index_count", C.c_uint32), ("first_index", C.c_uint32), ("mesh", C.c_uint32),
                ("material", C.c_uint32), ("bounds", SvrBounds), ("transform", C.c_float * 16)]


class SvrSamplerDesc(C.Structure):
    _fields_ = [("mag_filter", C.c_int32), ("min_filter", C.c_int32), ("mipmap_mode", C.c_int32),
                ("min_lod", C.c_float), ("max_lod", C.c_float)]


class SvrStats(C.Structure):  # src/vk_engine.h:16-22 + extensions
    _fields_ = [("frame_time", C.c_float), ("triangle_count", C.c_int32), ("drawcall_count", C.c_int32),
                ("scene_update_time", C.c_float), ("mesh_draw_time", C.c_float),
                ("gpu_time_ms", C.c_float), ("culled_draws", C.c_uint32), ("timed_passes", C.c_uint32),
                ("shaded_fragments", C.c_uint64), ("rasterized_fragments", C.c_uint64),
                ("binned_triangles", C.c_uint64), ("bin_entries", C.c_uint64),
                ("geometry_ms", C.c_float), ("binning_ms", C.c_float), ("tile_ms", C.c_float),
                ("replayed_passes", C.c_uint32)]


class SvrConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("color_format", C.c_int32), ("reserved", C.c_uint32 * 4)]


VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("uv_x", "<f4"), ("normal", "<f4", 3),
                         ("uv_y", "<f4"), ("color", "<f4", 4)])
RENDER_OBJECT_DTYPE = np.dtype([("index_count", "<u4"), ("first_index", "<u4"), ("mesh", "<u4"),
                                ("material", "<u4"), ("origin", "<f4", 3), ("sphere_radius", "<f4"),
                                ("extents", "<f4", 3), ("transform", "<f4", 16)])
assert VERTEX_DTYPE.itemsize == C.sizeof(SvrVertex) == 48
assert RENDER_OBJECT_DTYPE.itemsize == C.sizeof(SvrRenderObject) == 108
assert C.sizeof(SvrSceneData) == 240
assert C.sizeof(SvrBounds) == 28

COLOR_RGBA16F, COLOR_RGBA8 = 0, 1
PASS_MAIN_COLOR, PASS_TRANSPARENT, PASS_OTHER = 0, 1, 2
FILTER_NEAREST, FILTER_LINEAR = 0, 1
MIPMAP_NEAREST, MIPMAP_LINEAR = 0, 1
LOD_CLAMP_NONE = 1000.0
OPT_COUNT_FRAGMENTS = 1
OPT_KERNEL_TIMING = 2
OPT_TILE_CYCLES = 3
OPT_TUNING = 4
OPT_QUEUE_CAPS = 5
OPT_DEVICE_FLATTEN = 6
BACKGROUND_GRADIENT, BACKGROUND_SKY = 0, 1
VS_COLORED_TRIANGLE, VS_COLORED_TRIANGLE_MESH = 1, 2
SWAPCHAIN_B8G8R8A8, SWAPCHAIN_R8G8B8A8 = 0, 1
GRADIENT_DEFAULT = (1.0, 1.0, 1.0, 1.0) * 2 + (0.0,) * 8       # src/vk_engine.cpp:981-982
SKY_DEFAULT = (0.1, 0.2, 0.4, 0.97) + (0.0,) * 12               # src/vk_engine.cpp:988

# every symbol include/svr.h declares
SYMBOLS = ["svr_create", "svr_destroy", "svr_set_stream", "svr_bind_targets", "svr_get_targets",
           "svr_upload_mesh", "svr_destroy_mesh", "svr_create_image", "svr_destroy_image",
           "svr_read_image_level", "svr_create_sampler", "svr_write_material", "svr_clear_color",
           "svr_draw_background", "svr_copy_to_swapchain", "svr_read_swapchain",
           "svr_set_scissor", "svr_set_row_interleave", "svr_set_present_status", "svr_draw_geometry", "svr_draw_colored_triangle", "svr_draw_tex_image",
           "svr_run_mesh_vert", "svr_run_vertex_shader", "svr_set_option", "svr_debug_trace_pixel", "svr_debug_read_trace", "svr_debug_read_bins", "svr_debug_read_tile_cycles", "svr_debug_rcp_sweep", "svr_get_row_costs", "svr_sync", "svr_read_color", "svr_read_depth", "svr_get_stats",
           "svr_last_error", "svr_backend_name"]
# include/svr_draw_list.h: retained draw lists, HIP library only (the oracle exports exactly SYMBOLS)
DRAW_LIST_SYMBOLS = ["svr_create_draw_list", "svr_update_draw_list", "svr_destroy_draw_list", "svr_draw_list",
                     "svr_debug_read_records"]
# include/svr_ids.h: the object and primitive ID target, HIP library only
ID_SYMBOLS = ["svr_enable_ids", "svr_bind_id_target", "svr_get_id_target", "svr_read_ids", "svr_pick"]
# include/svr_attributes.h: attribute targets (barycentrics, UV, normal, albedo per pixel), HIP library only
ATTRIBUTE_SYMBOLS = ["svr_enable_attributes", "svr_bind_attribute_target", "svr_get_attribute_target", "svr_read_attribute"]
ATTR_BARY, ATTR_UV, ATTR_NORMAL, ATTR_ALBEDO, ATTR_ALL = 1, 2, 4, 8, 15
ATTR_FLOATS = {ATTR_BARY: 4, ATTR_UV: 2, ATTR_NORMAL: 4, ATTR_ALBEDO: 4}  # floats per texel
# include/svr_views.h: multiview passes, HIP library only
VIEWS_SYMBOLS = ["svr_draw_geometry_views", "svr_draw_list_views"]
MAX_VIEWS = 16
# include/svr_depth.h: depth-only passes, HIP library only
DEPTH_SYMBOLS = ["svr_draw_depth", "svr_draw_list_depth", "svr_draw_depth_views", "svr_draw_list_depth_views"]
# include/svr_occlusion.h: occlusion culling against a depth pyramid, HIP library only
OCCLUSION_SYMBOLS = ["svr_create_depth_pyramid", "svr_destroy_depth_pyramid", "svr_build_depth_pyramid",
                     "svr_set_occlusion_pyramid", "svr_read_depth_pyramid", "svr_get_occlusion_stats",
                     "svr_debug_read_occlusion"]
# include/svr_lighting.h: the deferred lighting pass, HIP library only
LIGHTING_SYMBOLS = ["svr_light_pass", "svr_debug_read_light_tiles"]
MAX_LIGHTS = 4096
# include/svr_load.h: the depth loadOp of geometry passes, HIP library only
LOAD_SYMBOLS = ["svr_set_depth_load_op", "svr_get_depth_load_op"]
DEPTH_CLEAR, DEPTH_LOAD = 0, 1
# include/svr_post.h: the HDR post pass (exposure, bloom, tone mapping), HIP library only
POST_SYMBOLS = ["svr_post_pass"]
POST_MAX_LEVELS = 8
TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
# include/svr_temporal.h: temporal antialiasing (history reprojection, neighbourhood clamp, blend), HIP library only
TEMPORAL_SYMBOLS = ["svr_temporal_resolve", "svr_debug_read_temporal_history"]
TEMPORAL_RESET, TEMPORAL_NO_CLAMP = 1, 2
# include/svr_ambient.h: screen-space ambient occlusion over the G-buffer, HIP library only
AMBIENT_SYMBOLS = ["svr_ambient_pass", "svr_bind_ambient_target", "svr_get_ambient_target", "svr_read_ambient",
                   "svr_set_light_ambient_occlusion", "svr_debug_read_ambient_raw"]
AMBIENT_NO_BLUR = 1
AMBIENT_MAX_REACH, AMBIENT_TAPS = 16, 8
# include/svr_exposure.h: auto-exposure (a luminance histogram and an adapted exposure in device memory), HIP library only
EXPOSURE_SYMBOLS = ["svr_meter_exposure", "svr_reset_exposure", "svr_set_post_auto_exposure", "svr_read_exposure",
                    "svr_debug_read_exposure_histogram", "svr_get_exposure_state"]
EXPOSURE_BINS = 256
# include/svr_overlay.h: the UI overlay pass (2D triangle lists blended over the swapchain image), HIP library only
OVERLAY_SYMBOLS = ["svr_draw_overlay", "svr_debug_read_overlay_stats", "svr_overlay_font"]
OVERLAY_MAX_TRIANGLES, OVERLAY_MAX_CMDS, OVERLAY_MAX_TEXTURES, OVERLAY_MAX_TEXTURE_EXTENT = 65536, 4096, 16, 16384
OVERLAY_TEX_RGBA8, OVERLAY_TEX_A8 = 0, 1
OVERLAY_FONT_WHITE_X, OVERLAY_FONT_WHITE_Y = 92, 43
# include/svr_upscale.h: the upscaled present (bicubic magnification, anti-ringing clamp, adaptive sharpen), HIP library only
UPSCALE_SYMBOLS = ["svr_upscale_to_swapchain", "svr_read_upscaled"]
UPSCALE_NO_SHARPEN = 1
# include/svr_fog.h: the fog pass (height fog and sun shafts marched through the shadow map), HIP library only
FOG_SYMBOLS = ["svr_fog_pass"]
FOG_MAX_STEPS = 64
# include/svr_dof.h: the depth of field pass (a thin-lens blur gathered over the HDR colour target), HIP library only
DOF_SYMBOLS = ["svr_dof_pass"]
DOF_MAX_RADIUS = 16
# include/svr_motion.h: the camera motion blur pass (streaks gathered along the reprojected velocity), HIP library only
MOTION_SYMBOLS = ["svr_motion_blur_pass"]
MOTION_MAX_BLUR = 16
# include/svr_reflect.h: the reflection pass (screen-space rays marched through the depth target), HIP library only
REFLECT_SYMBOLS = ["svr_reflect_pass"]
REFLECT_MAX_STEPS, REFLECT_MAX_REFINE = 64, 8
DRAW_DESC_BYTES, WAVE_CHUNK_BYTES = 192, 8  # the records svr_debug_read_records returns (csrc/svr_device.h)


class SvrViewTargets(C.Structure):  # include/svr_views.h
    _fields_ = [("color", C.c_void_p), ("depth", C.c_void_p), ("ids", C.c_void_p), ("clear_rgba", C.POINTER(C.c_float))]


class SvrOcclusionStats(C.Structure):  # include/svr_occlusion.h
    _fields_ = [("chunks_tested", C.c_uint64), ("chunks_culled", C.c_uint64), ("triangles_culled", C.c_uint64)]


class SvrPointLight(C.Structure):  # include/svr_lighting.h
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 3), ("intensity", C.c_float)]


class SvrLightPass(C.Structure):  # include/svr_lighting.h
    _fields_ = [("inv_viewproj", C.c_float * 16), ("ambient_color", C.c_float * 4), ("sunlight_direction", C.c_float * 4),
                ("sunlight_color", C.c_float * 4), ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("shadow_depth", C.c_void_p), ("shadow_width", C.c_uint32), ("shadow_height", C.c_uint32),
                ("shadow_viewproj", C.c_float * 16), ("shadow_bias", C.c_float)]


class SvrPostPass(C.Structure):  # include/svr_post.h
    _fields_ = [("exposure", C.c_float), ("bloom_threshold", C.c_float), ("bloom_intensity", C.c_float),
                ("bloom_levels", C.c_uint32), ("tonemap", C.c_uint32)]


class SvrTemporalPass(C.Structure):  # include/svr_temporal.h
    _fields_ = [("reproject", C.c_float * 16), ("blend", C.c_float), ("flags", C.c_uint32)]


class SvrAmbientPass(C.Structure):  # include/svr_ambient.h
    _fields_ = [("inv_viewproj", C.c_float * 16), ("radius", C.c_float), ("pixels_per_unit", C.c_float), ("bias", C.c_float),
                ("intensity", C.c_float), ("sharpness", C.c_float), ("flags", C.c_uint32)]


class SvrExposureMeter(C.Structure):  # include/svr_exposure.h
    _fields_ = [("key", C.c_float), ("low_fraction", C.c_float), ("high_fraction", C.c_float), ("min_exposure", C.c_float),
                ("max_exposure", C.c_float), ("adapt", C.c_float)]


class SvrExposureState(C.Structure):  # include/svr_exposure.h
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("mean_log2", C.c_float), ("counted", C.c_uint32),
                ("black", C.c_uint32), ("meters", C.c_uint32)]


class SvrOverlayVertex(C.Structure):  # include/svr_overlay.h
    _fields_ = [("pos", C.c_float * 2), ("uv", C.c_float * 2), ("col", C.c_uint32)]


class SvrOverlayCmd(C.Structure):  # include/svr_overlay.h
    _fields_ = [("clip_rect", C.c_float * 4), ("texture", C.c_uint32), ("vtx_offset", C.c_uint32), ("idx_offset", C.c_uint32),
                ("elem_count", C.c_uint32)]


class SvrOverlayTexture(C.Structure):  # include/svr_overlay.h
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("reserved", C.c_uint32)]


class SvrOverlayList(C.Structure):  # include/svr_overlay.h
    _fields_ = [("vertices", C.c_void_p), ("indices", C.c_void_p), ("cmds", C.c_void_p), ("textures", C.c_void_p),
                ("n_vertices", C.c_uint32), ("n_indices", C.c_uint32), ("n_cmds", C.c_uint32), ("n_textures", C.c_uint32),
                ("display_pos", C.c_float * 2), ("scale", C.c_float * 2)]


class SvrOverlayStats(C.Structure):  # include/svr_overlay.h
    _fields_ = [("triangles", C.c_uint32), ("kept", C.c_uint32), ("tiles", C.c_uint32)]


class SvrUpscalePass(C.Structure):  # include/svr_upscale.h
    _fields_ = [("sharpness", C.c_float), ("flags", C.c_uint32)]


class SvrDofPass(C.Structure):  # include/svr_dof.h
    _fields_ = [("inv_z_scale", C.c_float), ("inv_z_bias", C.c_float), ("focus_distance", C.c_float), ("blur_scale", C.c_float),
                ("max_radius", C.c_float)]


class SvrMotionBlurPass(C.Structure):  # include/svr_motion.h
    _fields_ = [("reproject", C.c_float * 16), ("shutter", C.c_float), ("max_blur", C.c_float)]


class SvrReflectPass(C.Structure):  # include/svr_reflect.h
    _fields_ = [("viewproj", C.c_float * 16), ("inv_viewproj", C.c_float * 16), ("camera_position", C.c_float * 3),
                ("inv_z_scale", C.c_float), ("inv_z_bias", C.c_float), ("max_distance", C.c_float), ("steps", C.c_uint32),
                ("refine", C.c_uint32), ("thickness", C.c_float), ("f0", C.c_float), ("intensity", C.c_float),
                ("distance_fade", C.c_float), ("edge_width", C.c_float), ("resolve", C.c_uint32), ("depth_tolerance", C.c_float),
                ("frame_index", C.c_uint32)]


class SvrFogPass(C.Structure):  # include/svr_fog.h
    _fields_ = [("inv_viewproj", C.c_float * 16), ("camera_position", C.c_float * 3), ("density", C.c_float),
                ("height_falloff", C.c_float), ("height_base", C.c_float), ("max_distance", C.c_float), ("steps", C.c_uint32),
                ("fog_color", C.c_float * 3), ("anisotropy", C.c_float), ("sunlight_direction", C.c_float * 4),
                ("sun_color", C.c_float * 3), ("edge_sharpness", C.c_float), ("shadow_depth", C.c_void_p),
                ("shadow_width", C.c_uint32), ("shadow_height", C.c_uint32), ("shadow_viewproj", C.c_float * 16),
                ("shadow_bias", C.c_float), ("frame_index", C.c_uint32)]


OVERLAY_VERTEX_DTYPE = np.dtype([("pos", "<f4", 2), ("uv", "<f4", 2), ("col", "<u4")])
OVERLAY_CMD_DTYPE = np.dtype([("clip_rect", "<f4", 4), ("texture", "<u4"), ("vtx_offset", "<u4"), ("idx_offset", "<u4"), ("elem_count", "<u4")])
assert OVERLAY_VERTEX_DTYPE.itemsize == C.sizeof(SvrOverlayVertex) == 20 and OVERLAY_CMD_DTYPE.itemsize == C.sizeof(SvrOverlayCmd) == 32

POINT_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("radius", "<f4"), ("color", "<f4", 3), ("intensity", "<f4")])
assert POINT_LIGHT_DTYPE.itemsize == C.sizeof(SvrPointLight) == 32


class SvrError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"svr error {code}: {text}")
        self.code = code


class SvrLib:
    """One loaded shared library exporting the svr.h ABI."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.lib = C.CDLL(path)
        L = self.lib
        P = C.c_void_p
        L.svr_last_error.restype = C.c_char_p
        L.svr_backend_name.restype = C.c_char_p
        L.svr_destroy.restype = None
        L.svr_create.argtypes = [C.POINTER(SvrConfig), C.POINTER(P)]
        L.svr_destroy.argtypes = [P]
        L.svr_set_stream.argtypes = [P, P]
        L.svr_bind_targets.argtypes = [P, P, P]
        L.svr_get_targets.argtypes = [P, C.POINTER(P), C.POINTER(P)]
        L.svr_upload_mesh.argtypes = [P, P, C.c_size_t, P, C.c_size_t, C.POINTER(C.c_uint32)]
        L.svr_destroy_mesh.argtypes = [P, C.c_uint32]
        L.svr_create_image.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
        L.svr_destroy_image.argtypes = [P, C.c_uint32]
        L.svr_read_image_level.argtypes = [P, C.c_uint32, C.c_uint32, P, C.c_size_t,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.svr_create_sampler.argtypes = [P, C.POINTER(SvrSamplerDesc), C.POINTER(C.c_uint32)]
        L.svr_write_material.argtypes = [P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.svr_clear_color.argtypes = [P, C.POINTER(C.c_float)]
        L.svr_draw_background.argtypes = [P, C.c_int, C.POINTER(C.c_float)]
        L.svr_copy_to_swapchain.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_int]
        L.svr_read_swapchain.argtypes = [P, C.c_uint32, C.c_uint32, C.c_int, P, C.c_size_t]
        L.svr_set_scissor.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        if hasattr(L, "svr_set_row_interleave"):  # tools/ab_libs.py also loads builds that predate these
            L.svr_set_row_interleave.argtypes = [P, C.c_uint32, C.c_uint32]
            L.svr_set_present_status.argtypes = [P, P]
        L.svr_draw_geometry.argtypes = [P, C.POINTER(SvrSceneData), P, C.c_size_t, P, C.c_size_t,
                                        C.POINTER(SvrStats)]
        L.svr_draw_colored_triangle.argtypes = [P, C.POINTER(SvrStats)]
        L.svr_draw_tex_image.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                         C.c_uint32, C.c_uint32, C.POINTER(SvrStats)]
        L.svr_run_mesh_vert.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                        C.POINTER(SvrSceneData), C.c_uint32, P, P]
        if hasattr(L, "svr_run_vertex_shader"):  # tools/ab_libs.py also loads builds that predate it
            L.svr_run_vertex_shader.argtypes = [P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), P, P]
        L.svr_set_option.argtypes = [P, C.c_int, C.c_int64]
        L.svr_debug_trace_pixel.argtypes = [P, C.c_int, C.c_int]
        L.svr_debug_read_trace.argtypes = [P, P]
        L.svr_debug_read_bins.argtypes = [P, P, C.c_size_t, C.POINTER(C.c_uint32)]
        L.svr_debug_read_tile_cycles.argtypes = [P, P, C.c_size_t]
        if hasattr(L, "svr_get_row_costs"):
            L.svr_get_row_costs.argtypes = [P, P, C.c_size_t, P, P, P]
        if hasattr(L, "svr_debug_rcp_sweep"):  # tools/ab_libs.py also loads builds that predate it
            L.svr_debug_rcp_sweep.argtypes = [P, C.c_int, C.c_uint64, C.c_uint64, P, P, P]
        L.svr_sync.argtypes = [P]
        L.svr_read_color.argtypes = [P, P, C.c_size_t, C.c_int]
        L.svr_read_depth.argtypes = [P, P, C.c_size_t]
        L.svr_get_stats.argtypes = [P, C.POINTER(SvrStats)]
        self.has_draw_lists = hasattr(L, "svr_create_draw_list")
        if self.has_draw_lists:
            L.svr_create_draw_list.argtypes = [P, P, C.c_size_t, P, C.c_size_t, C.POINTER(C.c_uint32)]
            L.svr_update_draw_list.argtypes = [P, C.c_uint32, C.c_size_t, P, C.c_size_t]
            L.svr_destroy_draw_list.argtypes = [P, C.c_uint32]
            L.svr_draw_list.argtypes = [P, C.c_uint32, C.POINTER(SvrSceneData), C.POINTER(SvrStats)]
            L.svr_debug_read_records.argtypes = [P, P, C.c_size_t, P, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        self.has_views = hasattr(L, "svr_draw_geometry_views")
        if self.has_views:
            L.svr_draw_geometry_views.argtypes = [P, C.c_uint32, P, C.POINTER(SvrViewTargets), P, C.c_size_t, P, C.c_size_t,
                                                  C.POINTER(SvrStats)]
            L.svr_draw_list_views.argtypes = [P, C.c_uint32, C.c_uint32, P, C.POINTER(SvrViewTargets), C.POINTER(SvrStats)]
        self.has_depth = hasattr(L, "svr_draw_depth")
        if self.has_depth:
            L.svr_draw_depth.argtypes = [P, C.POINTER(SvrSceneData), P, C.c_size_t, C.POINTER(SvrStats)]
            L.svr_draw_list_depth.argtypes = [P, C.c_uint32, C.POINTER(SvrSceneData), C.POINTER(SvrStats)]
            L.svr_draw_depth_views.argtypes = [P, C.c_uint32, P, C.POINTER(SvrViewTargets), P, C.c_size_t, C.POINTER(SvrStats)]
            L.svr_draw_list_depth_views.argtypes = [P, C.c_uint32, C.c_uint32, P, C.POINTER(SvrViewTargets), C.POINTER(SvrStats)]
        self.has_occlusion = hasattr(L, "svr_create_depth_pyramid")
        if self.has_occlusion:
            L.svr_create_depth_pyramid.argtypes = [P, C.POINTER(C.c_uint32)]
            L.svr_destroy_depth_pyramid.argtypes = [P, C.c_uint32]
            L.svr_build_depth_pyramid.argtypes = [P, C.c_uint32, P]
            L.svr_set_occlusion_pyramid.argtypes = [P, C.c_uint32]
            L.svr_read_depth_pyramid.argtypes = [P, C.c_uint32, C.c_uint32, P, C.c_size_t, C.POINTER(C.c_uint32)]
            L.svr_get_occlusion_stats.argtypes = [P, C.POINTER(SvrOcclusionStats)]
            L.svr_debug_read_occlusion.argtypes = [P, P, C.c_size_t, C.POINTER(C.c_uint32)]
        self.has_ids = hasattr(L, "svr_enable_ids")
        if self.has_ids:
            L.svr_enable_ids.argtypes = [P, C.c_int]
            L.svr_bind_id_target.argtypes = [P, P]
            L.svr_get_id_target.argtypes = [P, C.POINTER(P)]
            L.svr_read_ids.argtypes = [P, P, C.c_size_t]
            L.svr_pick.argtypes = [P, C.c_uint32, C.c_uint32, P]
        self.has_attributes = hasattr(L, "svr_enable_attributes")
        if self.has_attributes:
            L.svr_enable_attributes.argtypes = [P, C.c_uint32]
            L.svr_bind_attribute_target.argtypes = [P, C.c_int, P]
            L.svr_get_attribute_target.argtypes = [P, C.c_int, C.POINTER(P)]
            L.svr_read_attribute.argtypes = [P, C.c_int, P, C.c_size_t]
        self.has_lighting = hasattr(L, "svr_light_pass")
        if self.has_lighting:
            L.svr_light_pass.argtypes = [P, C.POINTER(SvrLightPass)]
            L.svr_debug_read_light_tiles.argtypes = [P, P, C.c_size_t, C.POINTER(C.c_uint32)]
        self.has_post = hasattr(L, "svr_post_pass")
        if self.has_post:
            L.svr_post_pass.argtypes = [P, C.POINTER(SvrPostPass)]
        self.has_temporal = hasattr(L, "svr_temporal_resolve")
        if self.has_temporal:
            L.svr_temporal_resolve.argtypes = [P, C.POINTER(SvrTemporalPass)]
            L.svr_debug_read_temporal_history.argtypes = [P, P, C.c_size_t, C.POINTER(C.c_uint32)]
        self.has_ambient = hasattr(L, "svr_ambient_pass")
        if self.has_ambient:
            L.svr_ambient_pass.argtypes = [P, C.POINTER(SvrAmbientPass)]
            L.svr_bind_ambient_target.argtypes = [P, P]
            L.svr_get_ambient_target.argtypes = [P, C.POINTER(P)]
            L.svr_read_ambient.argtypes = [P, P, C.c_size_t]
            L.svr_set_light_ambient_occlusion.argtypes = [P, C.c_int]
            L.svr_debug_read_ambient_raw.argtypes = [P, P, C.c_size_t]
        self.has_exposure = hasattr(L, "svr_meter_exposure")
        if self.has_exposure:
            L.svr_meter_exposure.argtypes = [P, C.POINTER(SvrExposureMeter)]
            L.svr_reset_exposure.argtypes = [P]
            L.svr_set_post_auto_exposure.argtypes = [P, C.c_int]
            L.svr_read_exposure.argtypes = [P, C.POINTER(SvrExposureState)]
            L.svr_debug_read_exposure_histogram.argtypes = [P, P, C.c_size_t]
            L.svr_get_exposure_state.argtypes = [P, C.POINTER(P)]
        self.has_overlay = hasattr(L, "svr_draw_overlay")
        if self.has_overlay:
            L.svr_draw_overlay.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(SvrOverlayList)]
            L.svr_debug_read_overlay_stats.argtypes = [P, C.POINTER(SvrOverlayStats)]
            L.svr_overlay_font.argtypes = [C.POINTER(C.POINTER(C.c_uint8))] + [C.POINTER(C.c_uint32)] * 6
        self.has_upscale = hasattr(L, "svr_upscale_to_swapchain")
        if self.has_upscale:
            L.svr_upscale_to_swapchain.argtypes = [P, C.POINTER(SvrUpscalePass), P, C.c_uint32, C.c_uint32, C.c_int]
            L.svr_read_upscaled.argtypes = [P, C.POINTER(SvrUpscalePass), C.c_uint32, C.c_uint32, C.c_int, P, C.c_size_t]
        self.has_dof = hasattr(L, "svr_dof_pass")
        if self.has_dof:
            L.svr_dof_pass.argtypes = [P, C.POINTER(SvrDofPass)]
        self.has_motion = hasattr(L, "svr_motion_blur_pass")
        if self.has_motion:
            L.svr_motion_blur_pass.argtypes = [P, C.POINTER(SvrMotionBlurPass)]
        self.has_reflect = hasattr(L, "svr_reflect_pass")
        if self.has_reflect:
            L.svr_reflect_pass.argtypes = [P, C.POINTER(SvrReflectPass)]
        self.has_fog = hasattr(L, "svr_fog_pass")
        if self.has_fog:
            L.svr_fog_pass.argtypes = [P, C.POINTER(SvrFogPass)]
        self.has_depth_load = hasattr(L, "svr_set_depth_load_op")
        if self.has_depth_load:
            L.svr_set_depth_load_op.argtypes = [P, C.c_int]
            L.svr_get_depth_load_op.argtypes = [P, C.POINTER(C.c_int)]

    @property
    def backend(self):
        return self.lib.svr_backend_name().decode()

    def check(self, rc):
        if rc != 0:
            raise SvrError(rc, self.lib.svr_last_error().decode(errors="replace"))

    def create(self, width, height, color_format=COLOR_RGBA16F, device=0):
        return Renderer(self, width, height, color_format, device)


def overlay_device_ptr(x):
    """a device address: an int, None, or anything with data_ptr() (a torch tensor)"""
    if x is None:
        return None
    return C.c_void_p(int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


def overlay_font(lib):
    """svr_overlay_font -> (uint8 [height, width] A8 atlas, cell_w, cell_h, first_char, n_chars); needs no device"""
    if not getattr(lib, "has_overlay", False):
        raise SvrError(-5, f"{lib.backend} has no overlay pass (include/svr_overlay.h)")
    a8 = C.POINTER(C.c_uint8)()
    v = [C.c_uint32() for _ in range(6)]
    lib.check(lib.lib.svr_overlay_font(C.byref(a8), *[C.byref(x) for x in v]))
    w, h, cw, ch, first, n = [x.value for x in v]
    return np.ctypeslib.as_array(a8, shape=(h, w)).copy(), cw, ch, first, n


def _f4(a):
    return (C.c_float * 4)(*[float(x) for x in a])


def _f16m(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(16))
    return (C.c_float * 16)(*a.tolist())


def _set_shadow(p, shadow_ptr, shadow_size, shadow_viewproj, shadow_bias):
    """the five shadow fields of an SvrLightPass or SvrFogPass; without a map they stay zero"""
    if shadow_ptr:
        p.shadow_depth = C.c_void_p(shadow_ptr)
        p.shadow_width, p.shadow_height = int(shadow_size[0]), int(shadow_size[1])
        p.shadow_viewproj = _f16m(shadow_viewproj)
        p.shadow_bias = float(shadow_bias)


def fog_struct(inv_viewproj, camera_position, density, height_falloff=0.0, height_base=0.0, max_distance=100.0, steps=16,
               fog_color=(0.5, 0.6, 0.7), sun_dir=(0.0, 1.0, 0.0, 0.0), sun_color=(0.0, 0.0, 0.0), anisotropy=0.0, shadow_ptr=None,
               shadow_size=(0, 0), shadow_viewproj=None, shadow_bias=0.0, edge_sharpness=1.0, frame_index=0):
    """an SvrFogPass (include/svr_fog.h) from Python values; sun_dir may have 3 or 4 components"""
    p = SvrFogPass()
    p.inv_viewproj = _f16m(inv_viewproj)
    p.camera_position = (C.c_float * 3)(*[float(x) for x in camera_position])
    p.density, p.height_falloff, p.height_base, p.max_distance = float(density), float(height_falloff), float(height_base), float(max_distance)
    p.steps = int(steps)
    p.fog_color = (C.c_float * 3)(*[float(x) for x in fog_color])
    p.anisotropy = float(anisotropy)
    p.sunlight_direction = _f4((list(sun_dir) + [0.0])[:4])
    p.sun_color = (C.c_float * 3)(*[float(x) for x in list(sun_color)[:3]])
    p.edge_sharpness = float(edge_sharpness)
    _set_shadow(p, shadow_ptr, shadow_size, shadow_viewproj, shadow_bias)
    p.frame_index = int(frame_index) & 0xffffffff
    return p


def dof_struct(inv_z_scale, inv_z_bias, focus_distance, blur_scale, max_radius=DOF_MAX_RADIUS):
    """an SvrDofPass (include/svr_dof.h) from Python values; (inv_z_scale, inv_z_bias): glmath.dof_depth_terms(proj)"""
    return SvrDofPass(float(inv_z_scale), float(inv_z_bias), float(focus_distance), float(blur_scale), float(max_radius))


def motion_struct(reproject, shutter, max_blur=MOTION_MAX_BLUR):
    """an SvrMotionBlurPass (include/svr_motion.h) from Python values; reproject: 4 x 4 indexed [col][row] like glmath's
    matrices (glmath.temporal_reproject)"""
    p = SvrMotionBlurPass()
    p.reproject = _f16m(reproject)
    p.shutter = float(shutter)
    p.max_blur = float(max_blur)
    return p


def reflect_struct(viewproj, inv_viewproj, camera_position, inv_z_scale, inv_z_bias, max_distance=20.0, steps=16, refine=4, thickness=0.1,
                   f0=0.04, intensity=1.0, distance_fade=1.0, edge_width=16.0, resolve=1, depth_tolerance=0.05, frame_index=0):
    """an SvrReflectPass (include/svr_reflect.h) from Python values; the matrices: 4 x 4 indexed [col][row] like glmath's;
    (inv_z_scale, inv_z_bias): glmath.dof_depth_terms(proj)"""
    p = SvrReflectPass()
    p.viewproj = _f16m(viewproj)
    p.inv_viewproj = _f16m(inv_viewproj)
    p.camera_position = (C.c_float * 3)(*[float(x) for x in camera_position])
    p.inv_z_scale, p.inv_z_bias, p.max_distance = float(inv_z_scale), float(inv_z_bias), float(max_distance)
    p.steps, p.refine = int(steps), int(refine)
    p.thickness, p.f0, p.intensity, p.distance_fade, p.edge_width = float(thickness), float(f0), float(intensity), float(distance_fade), float(edge_width)
    p.resolve = int(resolve)
    p.depth_tolerance = float(depth_tolerance)
    p.frame_index = int(frame_index) & 0xffffffff
    return p


def scene_struct(view, proj, viewproj, ambient, sun_dir, sun_color):
    s = SvrSceneData()
    s.view = _f16m(view)
    s.proj = _f16m(proj)
    s.viewproj = _f16m(viewproj)
    s.ambient_color = _f4(ambient)
    s.sunlight_direction = _f4(sun_dir)
    s.sunlight_color = _f4(sun_color)
    return s


class Renderer:
    """A context of one SvrLib: the VulkanEngine-shaped surface of the draw path."""

    def __init__(self, lib, width, height, color_format=COLOR_RGBA16F, device=0):
        self.lib = lib
        self.width, self.height, self.color_format = int(width), int(height), int(color_format)
        cfg = SvrConfig(device=device, width=width, height=height, color_format=color_format)
        h = C.c_void_p()
        lib.check(lib.lib.svr_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._clear_args, self._object_args = {}, {}

    def close(self):
        if self.h:
            self.lib.lib.svr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- resources
    def upload_mesh(self, indices, vertices):
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        vtx = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        out = C.c_uint32()
        self.lib.check(self.lib.lib.svr_upload_mesh(self.h, idx.ctypes.data, idx.size, vtx.ctypes.data,
                                                    vtx.size, C.byref(out)))
        return out.value

    def destroy_mesh(self, mesh):
        self.lib.check(self.lib.lib.svr_destroy_mesh(self.h, mesh))

    def create_image(self, rgba8, mipmapped=False):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        out = C.c_uint32()
        self.lib.check(self.lib.lib.svr_create_image(self.h, a.ctypes.data, a.shape[1], a.shape[0],
                                                     1 if mipmapped else 0, C.byref(out)))
        return out.value

    def destroy_image(self, image):
        self.lib.check(self.lib.lib.svr_destroy_image(self.h, image))

    def read_image_level(self, image, level):
        w, h = C.c_uint32(), C.c_uint32()
        self.lib.check(self.lib.lib.svr_read_image_level(self.h, image, level, None, 0, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 4), dtype=np.uint8)
        self.lib.check(self.lib.lib.svr_read_image_level(self.h, image, level, out.ctypes.data, out.nbytes,
                                                         C.byref(w), C.byref(h)))
        return out

    def create_sampler(self, mag=FILTER_NEAREST, minf=FILTER_NEAREST, mip=MIPMAP_NEAREST, min_lod=0.0,
                       max_lod=0.0):
        d = SvrSamplerDesc(mag, minf, mip, min_lod, max_lod)
        out = C.c_uint32()
        self.lib.check(self.lib.lib.svr_create_sampler(self.h, C.byref(d), C.byref(out)))
        return out.value

    def write_material(self, pass_type, color_factors, image, sampler, metal_rough=(1.0, 0.5, 0.0, 0.0)):
        out = C.c_uint32()
        self.lib.check(self.lib.lib.svr_write_material(self.h, pass_type, _f4(color_factors), _f4(metal_rough),
                                                       image, sampler, C.byref(out)))
        return out.value

    # -- per frame
    def set_stream(self, stream_handle):
        self.lib.check(self.lib.lib.svr_set_stream(self.h, C.c_void_p(stream_handle)))

    def bind_targets(self, color_ptr, depth_ptr):
        self.lib.check(self.lib.lib.svr_bind_targets(self.h, C.c_void_p(color_ptr), C.c_void_p(depth_ptr)))

    def get_targets(self):
        c, d = C.c_void_p(), C.c_void_p()
        self.lib.check(self.lib.lib.svr_get_targets(self.h, C.byref(c), C.byref(d)))
        return c.value, d.value

    def clear_color(self, rgba=(1.0, 1.0, 1.0, 1.0)):
        key = tuple(rgba)
        arr = self._clear_args.get(key)  # the same few colours frame after frame: keep their ctypes arrays
        if arr is None:
            if len(self._clear_args) > 16:
                self._clear_args.clear()
            arr = self._clear_args[key] = _f4(rgba)
        self.lib.check(self.lib.lib.svr_clear_color(self.h, arr))

    def draw_background(self, effect, data):
        """effect: BACKGROUND_GRADIENT / BACKGROUND_SKY; data: the 16 floats of ComputePushConstants."""
        arr = (C.c_float * 16)(*[float(v) for v in data])
        self.lib.check(self.lib.lib.svr_draw_background(self.h, int(effect), arr))

    def copy_to_swapchain(self, dst_ptr, width, height, fmt=0):
        self.lib.check(self.lib.lib.svr_copy_to_swapchain(self.h, C.c_void_p(dst_ptr), width, height, fmt))

    def read_swapchain(self, width, height, fmt=0):
        out = np.empty((height, width, 4), dtype=np.uint8)
        self.lib.check(self.lib.lib.svr_read_swapchain(self.h, width, height, fmt, out.ctypes.data, out.nbytes))
        return out

    def set_scissor(self, x, y, w, h):
        self.lib.check(self.lib.lib.svr_set_scissor(self.h, x, y, w, h))

    def set_row_interleave(self, stride, offset):
        """of the scissor's 32-row tile rows render those with index % stride == offset (1, 0: all)"""
        self.lib.check(self.lib.lib.svr_set_row_interleave(self.h, stride, offset))

    def set_present_status(self, status_ptr):
        """device word (oracle: host word) every copy_to_swapchain reports to: 1 = void, awaiting the replay"""
        self.lib.check(self.lib.lib.svr_set_present_status(self.h, C.c_void_p(status_ptr)))

    def _objects(self, a):
        """(address, count) of a RenderObject list; arrays of the right kind are passed as they are, and their address is
        remembered (ndarray.ctypes builds an object per access: microseconds that count against a 50-us band)."""
        if a is None:
            return 0, 0
        if not (isinstance(a, np.ndarray) and a.dtype == RENDER_OBJECT_DTYPE and a.flags.c_contiguous):
            a = np.ascontiguousarray(a, dtype=RENDER_OBJECT_DTYPE)
            self._keep = (getattr(self, "_keep", ()) + (a,))[-2:]  # alive for the duration of the call
            return a.ctypes.data, a.size
        hit = self._object_args.get(id(a))
        if hit is None or hit[0] is not a:
            if len(self._object_args) > 8:
                self._object_args.clear()
            hit = self._object_args[id(a)] = (a, a.ctypes.data, a.size)
        return hit[1], hit[2]

    def draw_geometry(self, scene, opaque, transparent=None):
        op, n_op = self._objects(opaque)
        tr, n_tr = self._objects(transparent)
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_geometry(self.h, C.byref(scene), op, n_op, tr, n_tr, C.byref(st)))
        return st

    # -- retained draw lists (include/svr_draw_list.h)
    def _need_draw_lists(self):
        if not self.lib.has_draw_lists:
            raise SvrError(-5, f"{self.lib.backend} has no draw lists (include/svr_draw_list.h)")

    def create_draw_list(self, opaque, transparent=None):
        """A DrawList holding copies of the two RenderObject arrays in device memory."""
        self._need_draw_lists()
        op = np.ascontiguousarray(opaque if opaque is not None else np.zeros(0, RENDER_OBJECT_DTYPE), dtype=RENDER_OBJECT_DTYPE)
        tr = np.ascontiguousarray(transparent if transparent is not None else np.zeros(0, RENDER_OBJECT_DTYPE), dtype=RENDER_OBJECT_DTYPE)
        out = C.c_uint32()
        self.lib.check(self.lib.lib.svr_create_draw_list(self.h, op.ctypes.data, op.size, tr.ctypes.data, tr.size, C.byref(out)))
        return DrawList(self, out.value, op.size, tr.size)

    def draw_list(self, scene, lst):
        """svr_draw_geometry over the list's objects; the three counts arrive with the pass (get_stats)."""
        st = SvrStats()
        handle = lst.handle if isinstance(lst, DrawList) else int(lst)
        self.lib.check(self.lib.lib.svr_draw_list(self.h, handle, C.byref(scene), C.byref(st)))
        return st

    # -- multiview passes (include/svr_views.h)
    def _view_args(self, scenes, color_ptr, depth_ptr, ids_ptr, clear_rgba):
        if not getattr(self.lib, "has_views", False):
            raise SvrError(-5, f"{self.lib.backend} has no multiview (include/svr_views.h)")
        scenes = list(scenes)
        arr = (SvrSceneData * max(len(scenes), 1))(*scenes)
        t = SvrViewTargets()
        t.color, t.depth, t.ids = C.c_void_p(color_ptr or None), C.c_void_p(depth_ptr or None), C.c_void_p(ids_ptr or None)
        if clear_rgba is not None:
            t.clear_rgba = (C.c_float * 4)(*[float(v) for v in clear_rgba])
        self._view_keep = (arr, t)  # alive for the duration of the call
        return len(scenes), arr, t

    def draw_views(self, scenes, color_ptr, depth_ptr, opaque, transparent=None, ids_ptr=None, clear_rgba=None):
        """svr_draw_geometry_views: scenes[k] draws layer k of the device targets (colour [K, H, W, C], depth [K, H, W],
        ids [K, H, W, 2] or None); clear_rgba None = colour LOAD"""
        n, arr, t = self._view_args(scenes, color_ptr, depth_ptr, ids_ptr, clear_rgba)
        op, n_op = self._objects(opaque)
        tr, n_tr = self._objects(transparent)
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_geometry_views(self.h, n, C.addressof(arr), C.byref(t), op, n_op, tr, n_tr, C.byref(st)))
        return st

    def draw_list_views(self, scenes, lst, color_ptr, depth_ptr, ids_ptr=None, clear_rgba=None):
        """svr_draw_list_views: draw_views over a retained list"""
        n, arr, t = self._view_args(scenes, color_ptr, depth_ptr, ids_ptr, clear_rgba)
        st = SvrStats()
        handle = lst.handle if isinstance(lst, DrawList) else int(lst)
        self.lib.check(self.lib.lib.svr_draw_list_views(self.h, handle, n, C.addressof(arr), C.byref(t), C.byref(st)))
        return st

    # -- depth-only passes (include/svr_depth.h)
    def _need_depth(self):
        if not getattr(self.lib, "has_depth", False):
            raise SvrError(-5, f"{self.lib.backend} has no depth-only passes (include/svr_depth.h)")

    def draw_depth(self, scene, opaque):
        """svr_draw_depth: the depth (and bound ID) target of draw_geometry(scene, opaque), without shading; colour untouched"""
        self._need_depth()
        op, n_op = self._objects(opaque)
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_depth(self.h, C.byref(scene), op, n_op, C.byref(st)))
        return st

    def draw_list_depth(self, scene, lst):
        """svr_draw_list_depth: draw_depth over a retained list's opaque objects"""
        self._need_depth()
        st = SvrStats()
        handle = lst.handle if isinstance(lst, DrawList) else int(lst)
        self.lib.check(self.lib.lib.svr_draw_list_depth(self.h, handle, C.byref(scene), C.byref(st)))
        return st

    def draw_depth_views(self, scenes, depth_ptr, opaque, ids_ptr=None):
        """svr_draw_depth_views: scenes[k] draws layer k of the device targets (depth [K, H, W], ids [K, H, W, 2] or None)"""
        self._need_depth()
        n, arr, t = self._view_args(scenes, None, depth_ptr, ids_ptr, None)
        op, n_op = self._objects(opaque)
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_depth_views(self.h, n, C.addressof(arr), C.byref(t), op, n_op, C.byref(st)))
        return st

    def draw_list_depth_views(self, scenes, lst, depth_ptr, ids_ptr=None):
        """svr_draw_list_depth_views: draw_depth_views over a retained list's opaque objects"""
        self._need_depth()
        n, arr, t = self._view_args(scenes, None, depth_ptr, ids_ptr, None)
        st = SvrStats()
        handle = lst.handle if isinstance(lst, DrawList) else int(lst)
        self.lib.check(self.lib.lib.svr_draw_list_depth_views(self.h, handle, n, C.addressof(arr), C.byref(t), C.byref(st)))
        return st

    # -- occlusion culling (include/svr_occlusion.h)
    def _need_occlusion(self):
        if not getattr(self.lib, "has_occlusion", False):
            raise SvrError(-5, f"{self.lib.backend} has no occlusion culling (include/svr_occlusion.h)")

    def create_depth_pyramid(self):
        """svr_create_depth_pyramid: a handle (int) of a pyramid sized for this context (all 0.0 until built)"""
        self._need_occlusion()
        h = C.c_uint32()
        self.lib.check(self.lib.lib.svr_create_depth_pyramid(self.h, C.byref(h)))
        return h.value

    def destroy_depth_pyramid(self, pyr):
        self._need_occlusion()
        self.lib.check(self.lib.lib.svr_destroy_depth_pyramid(self.h, int(pyr)))

    def build_depth_pyramid(self, pyr, depth_ptr=None):
        """svr_build_depth_pyramid from a device W x H float buffer (an address), or the context's depth target (None)"""
        self._need_occlusion()
        self.lib.check(self.lib.lib.svr_build_depth_pyramid(self.h, int(pyr), depth_ptr))

    def set_occlusion_pyramid(self, pyr):
        """svr_set_occlusion_pyramid: later passes cull against pyr; 0 = off"""
        self._need_occlusion()
        self.lib.check(self.lib.lib.svr_set_occlusion_pyramid(self.h, int(pyr)))

    def pyramid_levels(self, pyr):
        self._need_occlusion()
        n = C.c_uint32()
        rc = self.lib.lib.svr_read_depth_pyramid(self.h, int(pyr), 0, None, 0, C.byref(n))
        if rc not in (0, -1):
            self.lib.check(rc)
        return n.value

    def read_depth_pyramid(self, pyr, level):
        """level (1 ..) of pyr as uint32 bit patterns [ceil(H / 2^level), ceil(W / 2^level)] (fences)"""
        self._need_occlusion()
        lw, lh = -(-self.width // (1 << level)), -(-self.height // (1 << level))
        out = np.zeros((lh, lw), dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_read_depth_pyramid(self.h, int(pyr), int(level), out.ctypes.data, out.nbytes, None))
        return out

    def occlusion_stats(self):
        """svr_get_occlusion_stats: SvrOcclusionStats of the last instrumented pass"""
        self._need_occlusion()
        st = SvrOcclusionStats()
        self.lib.check(self.lib.lib.svr_get_occlusion_stats(self.h, C.byref(st)))
        return st

    def read_occlusion(self):
        """bool [n_chunks]: the chunks of the last pass that occlusion culling dropped, in read_records' order (fences)"""
        self._need_occlusion()
        n = C.c_uint32()
        L = self.lib.lib
        self.lib.check(L.svr_debug_read_occlusion(self.h, None, 0, C.byref(n)))
        words = np.zeros(max(1, (n.value + 31) // 32), dtype=np.uint32)
        self.lib.check(L.svr_debug_read_occlusion(self.h, words.ctypes.data, words.size, C.byref(n)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n.value]
        return bits.astype(bool)

    def read_records(self):
        """(DrawDesc records [n, 192] uint8, WaveChunk records [n, 2] uint32) the last pass ran with (fences)."""
        self._need_draw_lists()
        nd, nc = C.c_uint32(), C.c_uint32()
        L = self.lib.lib
        self.lib.check(L.svr_debug_read_records(self.h, None, 0, None, 0, C.byref(nd), C.byref(nc)))
        draws = np.zeros((nd.value, DRAW_DESC_BYTES), dtype=np.uint8)
        chunks = np.zeros((nc.value, 2), dtype=np.uint32)
        self.lib.check(L.svr_debug_read_records(self.h, draws.ctypes.data, draws.nbytes, chunks.ctypes.data, chunks.nbytes,
                                                C.byref(nd), C.byref(nc)))
        return draws, chunks

    def draw_colored_triangle(self):
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_colored_triangle(self.h, C.byref(st)))
        return st

    def draw_tex_image(self, mesh, first_index, index_count, render_matrix, image, sampler):
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_draw_tex_image(self.h, mesh, first_index, index_count,
                                                       _f16m(render_matrix), image, sampler, C.byref(st)))
        return st

    def run_mesh_vert(self, mesh, first_vertex, n_vertices, world, scene, material):
        clip = np.empty((n_vertices, 4), dtype=np.float32)
        var = np.empty((n_vertices, 8), dtype=np.float32)
        self.lib.check(self.lib.lib.svr_run_mesh_vert(self.h, mesh, first_vertex, n_vertices, _f16m(world),
                                                      C.byref(scene), material, clip.ctypes.data,
                                                      var.ctypes.data))
        return clip, var

    def run_vertex_shader(self, shader, mesh=0, first_vertex=0, n_vertices=3, render_matrix=None):
        """shader: VS_COLORED_TRIANGLE / VS_COLORED_TRIANGLE_MESH -> (clip [n,4], varyings [n,8])"""
        clip = np.empty((n_vertices, 4), dtype=np.float32)
        var = np.empty((n_vertices, 8), dtype=np.float32)
        mat = _f16m(render_matrix) if render_matrix is not None else None
        self.lib.check(self.lib.lib.svr_run_vertex_shader(self.h, shader, mesh, first_vertex, n_vertices, mat,
                                                          clip.ctypes.data, var.ctypes.data))
        return clip, var

    def set_option(self, option, value):
        self.lib.check(self.lib.lib.svr_set_option(self.h, option, value))

    def trace_pixel(self, x, y):
        self.lib.check(self.lib.lib.svr_debug_trace_pixel(self.h, int(x), int(y)))

    def read_bins(self):
        """(opaque counts, transparent counts) per 32x32 tile of the last pass, row-major."""
        n = C.c_uint32()
        self.lib.check(self.lib.lib.svr_debug_read_bins(self.h, None, 0, C.byref(n)))
        out = np.zeros(2 * n.value, dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_debug_read_bins(self.h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value], out[n.value:]

    def read_tile_cycles(self):
        n = C.c_uint32()
        self.lib.check(self.lib.lib.svr_debug_read_bins(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_debug_read_tile_cycles(self.h, out.ctypes.data, out.size))
        return out

    def row_costs(self):
        """(costs per tile row [uint32], first scissor row, scissor rows) of the last validated pass; empty before any."""
        n, y0, rows = C.c_uint32(), C.c_uint32(), C.c_uint32()
        out = np.zeros(512, dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_get_row_costs(self.h, out.ctypes.data, out.size, C.byref(n), C.byref(y0), C.byref(rows)))
        return out[:n.value].copy(), y0.value, rows.value

    def rcp_sweep(self, variant=0, first=0, count=1 << 32):
        """(mismatches, inputs on the refined path, first mismatching bit patterns) of svr_debug_rcp_sweep."""
        bad, fast = C.c_uint64(), C.c_uint64()
        pats = np.zeros(16, dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_debug_rcp_sweep(self.h, variant, first, count, C.byref(bad), C.byref(fast), pats.ctypes.data))
        return bad.value, fast.value, pats[:min(bad.value, 16)]

    def read_trace(self):
        out = np.zeros(64, dtype=np.float32)
        self.lib.check(self.lib.lib.svr_debug_read_trace(self.h, out.ctypes.data))
        return out

    def sync(self):
        self.lib.check(self.lib.lib.svr_sync(self.h))

    def read_color(self, as_rgba8=False):
        if as_rgba8 or self.color_format == COLOR_RGBA8:
            out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        else:
            out = np.empty((self.height, self.width, 4), dtype=np.uint16)  # fp16 bit patterns
        self.lib.check(self.lib.lib.svr_read_color(self.h, out.ctypes.data, out.nbytes, 1 if as_rgba8 else 0))
        return out

    def read_depth(self):
        out = np.empty((self.height, self.width), dtype=np.float32)
        self.lib.check(self.lib.lib.svr_read_depth(self.h, out.ctypes.data, out.nbytes))
        return out

    def get_stats(self):
        st = SvrStats()
        self.lib.check(self.lib.lib.svr_get_stats(self.h, C.byref(st)))
        return st

    # ---- the ID target (include/svr_ids.h)
    def _need_ids(self):
        if not getattr(self.lib, "has_ids", False):
            raise SvrError(-5, f"{self.lib.backend} has no ID target (include/svr_ids.h)")

    def enable_ids(self, on=True):
        """allocate (or free) the context's ID plane: geometry passes then write {object, primitive} per pixel"""
        self._need_ids()
        self.lib.check(self.lib.lib.svr_enable_ids(self.h, 1 if on else 0))

    def bind_id_target(self, ptr):
        """caller-owned device memory (width * height * 8 bytes) as the ID target; None/0 = back to the context's plane"""
        self._need_ids()
        self.lib.check(self.lib.lib.svr_bind_id_target(self.h, C.c_void_p(ptr or None)))

    def get_id_target(self):
        self._need_ids()
        p = C.c_void_p()
        self.lib.check(self.lib.lib.svr_get_id_target(self.h, C.byref(p)))
        return p.value

    def read_ids(self):
        """(H, W, 2) uint32: {object (1-based in the opaque array, 0 = none), primitive} per pixel"""
        self._need_ids()
        out = np.empty((self.height, self.width, 2), dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_read_ids(self.h, out.ctypes.data, out.nbytes))
        return out

    def pick(self, x, y):
        """(object, primitive) at pixel (x, y), or None where no opaque fragment won"""
        self._need_ids()
        out = (C.c_uint32 * 2)()
        self.lib.check(self.lib.lib.svr_pick(self.h, int(x), int(y), out))
        return None if out[0] == 0 else (int(out[0]), int(out[1]))

    # ---- attribute targets (include/svr_attributes.h)
    def _need_attributes(self):
        if not getattr(self.lib, "has_attributes", False):
            raise SvrError(-5, f"{self.lib.backend} has no attribute targets (include/svr_attributes.h)")

    def enable_attributes(self, mask=ATTR_ALL):
        """the context-owned planes are those of `mask` (ATTR_* bits) from here on; 0 frees them all"""
        self._need_attributes()
        self.lib.check(self.lib.lib.svr_enable_attributes(self.h, int(mask)))

    def bind_attribute_target(self, attr, ptr):
        """caller-owned device memory (width * height texels) as the plane of one attribute; None/0 = back to the context's"""
        self._need_attributes()
        self.lib.check(self.lib.lib.svr_bind_attribute_target(self.h, int(attr), C.c_void_p(ptr or None)))

    def get_attribute_target(self, attr):
        self._need_attributes()
        p = C.c_void_p()
        self.lib.check(self.lib.lib.svr_get_attribute_target(self.h, int(attr), C.byref(p)))
        return p.value

    def read_attribute(self, attr):
        """(H, W, 4) float32, UV: (H, W, 2): the plane of one attribute (all-zero texels: no opaque fragment won)"""
        self._need_attributes()
        out = np.empty((self.height, self.width, ATTR_FLOATS.get(int(attr), 4)), dtype=np.float32)
        self.lib.check(self.lib.lib.svr_read_attribute(self.h, int(attr), out.ctypes.data, out.nbytes))
        return out

    # ---- the deferred lighting pass (include/svr_lighting.h)
    def _need_lighting(self):
        if not getattr(self.lib, "has_lighting", False):
            raise SvrError(-5, f"{self.lib.backend} has no lighting pass (include/svr_lighting.h)")

    def light_pass(self, inv_viewproj, ambient, sun_dir, sun_color, lights=None, shadow_ptr=None, shadow_size=(0, 0),
                   shadow_viewproj=None, shadow_bias=0.0):
        """svr_light_pass: relight the opaque winners of the colour target from the depth target and the NORMAL and ALBEDO
        planes.  lights: POINT_LIGHT_DTYPE array or None; shadow_ptr: a device depth map of shadow_size = (width, height)
        drawn with shadow_viewproj, or None"""
        self._need_lighting()
        p = SvrLightPass()
        p.inv_viewproj = _f16m(inv_viewproj)
        p.ambient_color, p.sunlight_direction, p.sunlight_color = _f4(ambient), _f4(sun_dir), _f4(sun_color)
        arr = np.ascontiguousarray(lights if lights is not None else np.zeros(0, POINT_LIGHT_DTYPE), dtype=POINT_LIGHT_DTYPE).reshape(-1)
        p.lights, p.n_lights = (arr.ctypes.data if arr.size else None), arr.size
        _set_shadow(p, shadow_ptr, shadow_size, shadow_viewproj, shadow_bias)
        self.lib.check(self.lib.lib.svr_light_pass(self.h, C.byref(p)))

    def read_light_tiles(self):
        """uint32 [n_tiles]: the lights each 32x32 tile of the last lighting pass kept, row-major over its tile grid (fences)"""
        self._need_lighting()
        n = C.c_uint32()
        L = self.lib.lib
        self.lib.check(L.svr_debug_read_light_tiles(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self.lib.check(L.svr_debug_read_light_tiles(self.h, out.ctypes.data, out.size, C.byref(n)))
        return out

    # ---- the HDR post pass (include/svr_post.h)
    def post_pass(self, exposure=1.0, bloom_threshold=1.0, bloom_intensity=1.0, bloom_levels=4, tonemap=TONEMAP_ACES):
        """svr_post_pass: expose, bloom and tone-map the scissor's pixels of the RGBA16F colour target in place.
        bloom_levels: 0 .. POST_MAX_LEVELS (0: the tone map alone); tonemap: TONEMAP_*"""
        if not getattr(self.lib, "has_post", False):
            raise SvrError(-5, f"{self.lib.backend} has no post pass (include/svr_post.h)")
        p = SvrPostPass(float(exposure), float(bloom_threshold), float(bloom_intensity), int(bloom_levels), int(tonemap))
        self.lib.check(self.lib.lib.svr_post_pass(self.h, C.byref(p)))

    # ---- the fog pass (include/svr_fog.h)
    def fog_pass(self, inv_viewproj, camera_position, density, height_falloff=0.0, height_base=0.0, max_distance=100.0, steps=16,
                 fog_color=(0.5, 0.6, 0.7), sun_dir=(0.0, 1.0, 0.0, 0.0), sun_color=(0.0, 0.0, 0.0), anisotropy=0.0, shadow_ptr=None,
                 shadow_size=(0, 0), shadow_viewproj=None, shadow_bias=0.0, edge_sharpness=1.0, frame_index=0):
        """svr_fog_pass: height fog and sun shafts over the scissor's pixels of the RGBA16F colour target, in place.
        shadow_ptr: a device depth map of shadow_size = (width, height) drawn with shadow_viewproj, or None"""
        if not getattr(self.lib, "has_fog", False):
            raise SvrError(-5, f"{self.lib.backend} has no fog pass (include/svr_fog.h)")
        p = fog_struct(inv_viewproj, camera_position, density, height_falloff, height_base, max_distance, steps, fog_color, sun_dir,
                       sun_color, anisotropy, shadow_ptr, shadow_size, shadow_viewproj, shadow_bias, edge_sharpness, frame_index)
        self.lib.check(self.lib.lib.svr_fog_pass(self.h, C.byref(p)))

    # ---- the depth of field pass (include/svr_dof.h)
    def dof_pass(self, inv_z_scale, inv_z_bias, focus_distance, blur_scale, max_radius=DOF_MAX_RADIUS):
        """svr_dof_pass: a thin-lens blur over the scissor's pixels of the RGBA16F colour target, in place.  (inv_z_scale,
        inv_z_bias): glmath.dof_depth_terms(proj); blur_scale: the radius in pixels of a point at infinity
        (glmath.dof_blur_scale); no radius is larger than max_radius"""
        if not getattr(self.lib, "has_dof", False):
            raise SvrError(-5, f"{self.lib.backend} has no depth of field pass (include/svr_dof.h)")
        p = dof_struct(inv_z_scale, inv_z_bias, focus_distance, blur_scale, max_radius)
        self.lib.check(self.lib.lib.svr_dof_pass(self.h, C.byref(p)))

    # ---- the camera motion blur pass (include/svr_motion.h)
    def motion_blur_pass(self, reproject, shutter, max_blur=MOTION_MAX_BLUR):
        """svr_motion_blur_pass: streaks along the camera's motion over the scissor's pixels of the RGBA16F colour target,
        in place.  reproject: 4 x 4 indexed [col][row] like glmath's matrices (glmath.temporal_reproject, the one the
        temporal resolve takes); shutter: the open part of the frame interval; no streak reaches farther than max_blur
        pixels from its pixel"""
        if not getattr(self.lib, "has_motion", False):
            raise SvrError(-5, f"{self.lib.backend} has no motion blur pass (include/svr_motion.h)")
        p = motion_struct(reproject, shutter, max_blur)
        self.lib.check(self.lib.lib.svr_motion_blur_pass(self.h, C.byref(p)))

    # ---- the reflection pass (include/svr_reflect.h)
    def reflect_pass(self, viewproj, inv_viewproj, camera_position, inv_z_scale, inv_z_bias, max_distance=20.0, steps=16, refine=4, thickness=0.1,
                     f0=0.04, intensity=1.0, distance_fade=1.0, edge_width=16.0, resolve=1, depth_tolerance=0.05, frame_index=0):
        """svr_reflect_pass: screen-space reflections over the scissor's pixels of the RGBA16F colour target, in place: one
        ray per opaque pixel, marched `steps` samples over max_distance world units through the depth target and refined by
        `refine` bisections.  viewproj: what the G-buffer was drawn with, inv_viewproj its inverse, 4 x 4 indexed [col][row]
        like glmath's matrices; (inv_z_scale, inv_z_bias): glmath.dof_depth_terms(proj).  Needs the normal and albedo planes"""
        if not getattr(self.lib, "has_reflect", False):
            raise SvrError(-5, f"{self.lib.backend} has no reflection pass (include/svr_reflect.h)")
        p = reflect_struct(viewproj, inv_viewproj, camera_position, inv_z_scale, inv_z_bias, max_distance, steps, refine, thickness, f0, intensity,
                           distance_fade, edge_width, resolve, depth_tolerance, frame_index)
        self.lib.check(self.lib.lib.svr_reflect_pass(self.h, C.byref(p)))

    # ---- temporal antialiasing (include/svr_temporal.h)
    def _need_temporal(self):
        if not getattr(self.lib, "has_temporal", False):
            raise SvrError(-5, f"{self.lib.backend} has no temporal pass (include/svr_temporal.h)")

    def temporal_resolve(self, reproject, blend, flags=0):
        """svr_temporal_resolve: blend the scissor's pixels of the RGBA16F colour target with the reprojected, clamped
        history, in place.  reproject: 4 x 4 indexed [col][row] like glmath's matrices
        (glmath.temporal_reproject); blend: the current frame's weight in (0, 1]; flags: TEMPORAL_*"""
        self._need_temporal()
        p = SvrTemporalPass()
        p.reproject = _f16m(reproject)
        p.blend, p.flags = float(blend), int(flags)
        self.lib.check(self.lib.lib.svr_temporal_resolve(self.h, C.byref(p)))

    def read_temporal_history(self):
        """svr_debug_read_temporal_history -> (uint16 [H, W, 4] fp16 bit patterns the next resolve will read, valid)"""
        self._need_temporal()
        out = np.zeros((self.height, self.width, 4), np.uint16)
        valid = C.c_uint32(0)
        self.lib.check(self.lib.lib.svr_debug_read_temporal_history(self.h, out.ctypes.data, out.nbytes, C.byref(valid)))
        return out, bool(valid.value)

    # ---- ambient occlusion (include/svr_ambient.h)
    def _need_ambient(self):
        if not getattr(self.lib, "has_ambient", False):
            raise SvrError(-5, f"{self.lib.backend} has no ambient pass (include/svr_ambient.h)")

    def ambient_pass(self, inv_viewproj, radius, pixels_per_unit, bias=0.0, intensity=1.0, sharpness=0.05, flags=0):
        """svr_ambient_pass: the ambient factor of the scissor's pixels, from the depth target and the NORMAL plane, into
        the ambient target.  inv_viewproj: 4 x 4 indexed [col][row] like glmath's matrices; radius, bias: world units;
        pixels_per_unit: glmath.pixels_per_unit(proj, height); flags: AMBIENT_*"""
        self._need_ambient()
        p = SvrAmbientPass()
        p.inv_viewproj = _f16m(inv_viewproj)
        p.radius, p.pixels_per_unit, p.bias = float(radius), float(pixels_per_unit), float(bias)
        p.intensity, p.sharpness, p.flags = float(intensity), float(sharpness), int(flags)
        self.lib.check(self.lib.lib.svr_ambient_pass(self.h, C.byref(p)))

    def bind_ambient_target(self, ptr):
        """caller-owned device memory (width * height floats, 16-byte aligned) as the ambient target; None/0 = the context's"""
        self._need_ambient()
        self.lib.check(self.lib.lib.svr_bind_ambient_target(self.h, C.c_void_p(ptr or None)))

    def get_ambient_target(self):
        self._need_ambient()
        p = C.c_void_p()
        self.lib.check(self.lib.lib.svr_get_ambient_target(self.h, C.byref(p)))
        return p.value

    def read_ambient(self):
        """(H, W) float32: the current ambient target (fences)"""
        self._need_ambient()
        out = np.empty((self.height, self.width), dtype=np.float32)
        self.lib.check(self.lib.lib.svr_read_ambient(self.h, out.ctypes.data, out.nbytes))
        return out

    def read_ambient_raw(self):
        """svr_debug_read_ambient_raw -> (H, W, 2) float32: the (a, 1/w) scratch plane of the last passes (fences)"""
        self._need_ambient()
        out = np.empty((self.height, self.width, 2), dtype=np.float32)
        self.lib.check(self.lib.lib.svr_debug_read_ambient_raw(self.h, out.ctypes.data, out.nbytes))
        return out

    def set_light_ambient_occlusion(self, on=True):
        """later light_pass calls scale their ambient term by the ambient target current at their enqueue"""
        self._need_ambient()
        self.lib.check(self.lib.lib.svr_set_light_ambient_occlusion(self.h, 1 if on else 0))

    # ---- auto-exposure (include/svr_exposure.h)
    def _need_exposure(self):
        if not getattr(self.lib, "has_exposure", False):
            raise SvrError(-5, f"{self.lib.backend} has no auto-exposure (include/svr_exposure.h)")

    def meter_exposure(self, key=0.18, low_fraction=0.0, high_fraction=1.0, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, adapt=1.0):
        """svr_meter_exposure: histogram the luminance of the scissor's pixels of the RGBA16F colour target and move the
        device-resident exposure towards key / (the geometric mean of the pixels between the two fractions)"""
        self._need_exposure()
        m = SvrExposureMeter(float(key), float(low_fraction), float(high_fraction), float(min_exposure), float(max_exposure), float(adapt))
        self.lib.check(self.lib.lib.svr_meter_exposure(self.h, C.byref(m)))

    def reset_exposure(self):
        """svr_reset_exposure: the next accepted meter snaps, whatever its adapt"""
        self._need_exposure()
        self.lib.check(self.lib.lib.svr_reset_exposure(self.h))

    def set_post_auto_exposure(self, on=True):
        """later post_pass calls use their exposure times the state's, read on the device"""
        self._need_exposure()
        self.lib.check(self.lib.lib.svr_set_post_auto_exposure(self.h, 1 if on else 0))

    def read_exposure(self):
        """svr_read_exposure -> SvrExposureState behind everything enqueued so far (fences)"""
        self._need_exposure()
        st = SvrExposureState()
        self.lib.check(self.lib.lib.svr_read_exposure(self.h, C.byref(st)))
        return st

    def read_exposure_histogram(self):
        """svr_debug_read_exposure_histogram -> uint32 [EXPOSURE_BINS]: the last applied meter's bins (fences)"""
        self._need_exposure()
        out = np.zeros(EXPOSURE_BINS, dtype=np.uint32)
        self.lib.check(self.lib.lib.svr_debug_read_exposure_histogram(self.h, out.ctypes.data, out.nbytes))
        return out

    def exposure_state_ptr(self):
        """svr_get_exposure_state: the device address of the SvrExposureState, stable for the context's life"""
        self._need_exposure()
        p = C.c_void_p()
        self.lib.check(self.lib.lib.svr_get_exposure_state(self.h, C.byref(p)))
        return p.value

    # ---- the UI overlay pass (include/svr_overlay.h)
    def _need_overlay(self):
        if not getattr(self.lib, "has_overlay", False):
            raise SvrError(-5, f"{self.lib.backend} has no overlay pass (include/svr_overlay.h)")

    def draw_overlay(self, dst, width, height, fmt, vertices, indices, cmds, textures, display_pos=(0, 0), scale=(1, 1)):
        """svr_draw_overlay: blend a 2D triangle list over the width x height UNORM8 image at dst (a device pointer or a
        torch tensor), in submission order.  vertices: OVERLAY_VERTEX_DTYPE records; indices: uint16; cmds: OVERLAY_CMD_DTYPE
        records; textures: a sequence of (device pointer or torch tensor, width, height, OVERLAY_TEX_*)"""
        self._need_overlay()
        vertices = np.ascontiguousarray(vertices, dtype=OVERLAY_VERTEX_DTYPE)
        indices = np.ascontiguousarray(indices, dtype=np.uint16)
        cmds = np.ascontiguousarray(cmds, dtype=OVERLAY_CMD_DTYPE)
        table = (SvrOverlayTexture * max(len(textures), 1))()
        for i, (texels, w, h, f) in enumerate(textures):
            table[i] = SvrOverlayTexture(overlay_device_ptr(texels), int(w), int(h), int(f), 0)
        lst = SvrOverlayList(vertices.ctypes.data if vertices.size else None, indices.ctypes.data if indices.size else None,
                             cmds.ctypes.data if cmds.size else None, C.cast(table, C.c_void_p) if len(textures) else None,
                             vertices.size, indices.size, cmds.size, len(textures),
                             (C.c_float * 2)(*[float(v) for v in display_pos]), (C.c_float * 2)(*[float(v) for v in scale]))
        self.lib.check(self.lib.lib.svr_draw_overlay(self.h, overlay_device_ptr(dst), int(width), int(height), int(fmt), C.byref(lst)))

    def read_overlay_stats(self):
        """svr_debug_read_overlay_stats -> SvrOverlayStats of the last overlay that enqueued work (fences)"""
        self._need_overlay()
        st = SvrOverlayStats()
        self.lib.check(self.lib.lib.svr_debug_read_overlay_stats(self.h, C.byref(st)))
        return st

    # ---- the upscaled present (include/svr_upscale.h)
    def _need_upscale(self):
        if not getattr(self.lib, "has_upscale", False):
            raise SvrError(-5, f"{self.lib.backend} has no upscaled present (include/svr_upscale.h)")

    def upscale_to_swapchain(self, dst, width, height, fmt=0, sharpness=0.5, flags=0):
        """svr_upscale_to_swapchain: magnify the colour target into the width x height UNORM8 image at dst (a device
        pointer or a torch tensor) with a Catmull-Rom filter, an anti-ringing clamp and, unless UPSCALE_NO_SHARPEN, a
        contrast-adaptive sharpen"""
        self._need_upscale()
        p = SvrUpscalePass(float(sharpness), int(flags))
        self.lib.check(self.lib.lib.svr_upscale_to_swapchain(self.h, C.byref(p), overlay_device_ptr(dst), int(width), int(height), int(fmt)))

    def read_upscaled(self, width, height, fmt=0, sharpness=0.5, flags=0):
        """svr_read_upscaled -> uint8 [height, width, 4]: the same image, behind everything enqueued so far (fences)"""
        self._need_upscale()
        p = SvrUpscalePass(float(sharpness), int(flags))
        out = np.empty((height, width, 4), dtype=np.uint8)
        self.lib.check(self.lib.lib.svr_read_upscaled(self.h, C.byref(p), int(width), int(height), int(fmt), out.ctypes.data, out.nbytes))
        return out

    # ---- the depth loadOp (include/svr_load.h)
    def _need_depth_load(self):
        if not getattr(self.lib, "has_depth_load", False):
            raise SvrError(-5, f"{self.lib.backend} has no depth loadOp (include/svr_load.h)")

    def set_depth_load_op(self, op):
        """DEPTH_CLEAR (the default) or DEPTH_LOAD: later draw_geometry / draw_list passes start from the depth target as it
        stands, leave the ID target and the attribute planes alone, and write max(loaded, drawn) depth"""
        self._need_depth_load()
        self.lib.check(self.lib.lib.svr_set_depth_load_op(self.h, int(op)))

    def get_depth_load_op(self):
        self._need_depth_load()
        op = C.c_int()
        self.lib.check(self.lib.lib.svr_get_depth_load_op(self.h, C.byref(op)))
        return op.value


class DrawList:
    """A retained RenderObject list of one Renderer (svr_create_draw_list): opaque objects, then transparent ones."""

    def __init__(self, renderer, handle, n_opaque, n_transparent):
        self.renderer, self.handle = renderer, handle
        self.n_opaque, self.n_transparent = int(n_opaque), int(n_transparent)

    def __len__(self):
        return self.n_opaque + self.n_transparent

    def update(self, first, objects):
        """replace objects first .. first + len(objects) - 1 (indices over the opaque list, then the transparent one)"""
        a = np.ascontiguousarray(objects, dtype=RENDER_OBJECT_DTYPE).reshape(-1)
        r = self.renderer
        r.lib.check(r.lib.lib.svr_update_draw_list(r.h, self.handle, int(first), a.ctypes.data, a.size))

    def close(self):
        r = self.renderer
        if self.handle and r.h:
            r.lib.check(r.lib.lib.svr_destroy_draw_list(r.h, self.handle))
        self.handle = 0
