"""Loader of the in-tree libmcpt.so (host C++ + HIP kernels for gfx950).  No fallback: if the shared library is
missing or has no device to run on, the calls raise."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("MCPT_LIB") or os.path.join(CSRC, "libmcpt.so")     # MCPT_LIB: a differently tuned build (tools/)


class McptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmcpt error %d: %s" % (code, msg))
        self.code = code


class BvhInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("t", "Lc", "Lv", "Nc", "Nv", "Nr", "Level")]


class SceneInfo(C.Structure):
    _fields_ = [("num_faces", C.c_int32), ("num_materials", C.c_int32), ("num_lights", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32),
                ("eye", C.c_double * 3), ("look_at", C.c_double * 3), ("up", C.c_double * 3), ("fovy", C.c_double),
                ("bvh", BvhInfo)]


class Stats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_shadow", C.c_uint64), ("rays_bounce", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("shade_calls", C.c_uint64),
                ("samples", C.c_uint64), ("shadow_skipped", C.c_uint64), ("dom_rays", C.c_uint64),
                ("dom_node_visits", C.c_uint64), ("dom_tri_tests", C.c_uint64), ("ms_trace", C.c_double), ("ms_total", C.c_double),
                ("launches", C.c_int32), ("max_depth", C.c_int32)]

    @property
    def rays(self):
        return self.rays_primary + self.rays_shadow + self.rays_bounce

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["rays"] = self.rays
        return d


class RenderParams(C.Structure):
    _fields_ = [("spp", C.c_int32), ("seed", C.c_uint64), ("rank", C.c_int32), ("world", C.c_int32),
                ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("flags", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("num_faces", C.c_int64), ("v", C.POINTER(C.c_double)), ("vn", C.POINTER(C.c_double)), ("vt", C.POINTER(C.c_double)),
                ("material", C.POINTER(C.c_int32)), ("num_materials", C.c_int32), ("material_rec", C.POINTER(C.c_double)),
                ("material_names", C.POINTER(C.c_char_p)), ("num_lights", C.c_int32), ("light_material", C.POINTER(C.c_int32)),
                ("light_radiance", C.POINTER(C.c_double)), ("eye", C.c_double * 3), ("look_at", C.c_double * 3), ("up", C.c_double * 3),
                ("fovy", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class RenderSceneOptions(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("quiet", C.c_int32), ("output_prefix", C.c_char_p),
                ("load_flags", C.c_int32), ("output_flags", C.c_int32), ("checkpoint", C.c_char_p),
                ("checkpoint_parts", C.c_int32), ("reserved", C.c_int32),
                ("num_devices", C.c_int32), ("gather", C.c_int32), ("devices", C.POINTER(C.c_int32)),
                ("noise_target", C.c_double), ("time_budget_s", C.c_double),
                ("adaptive_min_spp", C.c_int32), ("reserved2", C.c_int32), ("abs_target", C.c_double)]


class AdaptiveParams(C.Structure):
    """mcpt_adaptive_params: the per-pixel stopping rule of an adaptive frame (mcpt_progressive_create_adaptive)"""
    _fields_ = [("rel_target", C.c_double), ("abs_target", C.c_double), ("min_spp", C.c_int32), ("reserved", C.c_int32)]


class DenoiseParams(C.Structure):
    """mcpt_denoise_params: the a-trous filter of mcpt_progressive_denoise (0 = the default)"""
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("sigma_l", C.c_double), ("sigma_z", C.c_double)]


class GuideParams(C.Structure):
    """mcpt_guide_params: the sample AOVs' count and the albedo sigma of mcpt_progressive_denoise_guided (0 = the default)"""
    _fields_ = [("samples", C.c_int32), ("reserved", C.c_int32), ("sigma_a", C.c_double)]


class Lens(C.Structure):
    """mcpt_lens: pixel-area jitter and a thin-lens aperture (mcpt_device_set_lens); all zero = the reference's pinhole"""
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32), ("aperture", C.c_double), ("focus_distance", C.c_double)]


class Environment(C.Structure):
    """mcpt_environment (mcpt.h: environment light)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_float)), ("scale", C.c_double), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class LightSampling(C.Structure):
    """mcpt_light_sampling (mcpt.h: light sampling)"""
    _fields_ = [("mode", C.c_int32), ("num_weights", C.c_int32), ("weights", C.POINTER(C.c_double))]


class FastInfo(C.Structure):
    """mcpt_fast_info: shape and origin of the culling hierarchy a device's fast walk walks (mcpt_device_fast_hierarchy)"""
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_tris", "enabled", "cw_stack_need", "max_depth", "builder", "clusters", "reserved")]


class UpdateInfo(C.Structure):
    """mcpt_update_info: what a geometry update did and what it took (mcpt_device_update_vertices)"""
    _fields_ = [("mode", C.c_int32), ("fast_enabled", C.c_int32), ("leaves_moved", C.c_int32), ("reserved", C.c_int32),
                ("ms_reference", C.c_double), ("ms_hierarchy", C.c_double), ("ms_tables", C.c_double), ("ms_total", C.c_double),
                ("cost_before", C.c_double), ("cost_after", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Shutter(C.Structure):
    """mcpt_shutter: the interval of a motion that is open, in `steps` time steps (mcpt_device_set_motion)"""
    _fields_ = [("open", C.c_double), ("close", C.c_double), ("steps", C.c_int32), ("reserved", C.c_int32)]


class CameraKey(C.Structure):
    """mcpt_camera_key: the camera of a motion's key 1"""
    _fields_ = [("eye", C.c_double * 3), ("look_at", C.c_double * 3), ("up", C.c_double * 3), ("fovy", C.c_double)]


class MotionInfo(C.Structure):
    """mcpt_motion_info: what the last motion frame's steps took (mcpt_device_motion_info)"""
    _fields_ = [("steps_run", C.c_int32), ("reserved", C.c_int32), ("ms_updates", C.c_double), ("max_cost_ratio", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Noise(C.Structure):
    """mcpt_noise: the frame summary of a progressive frame after `done` of `spp` samples"""
    _fields_ = [("done", C.c_int32), ("spp", C.c_int32), ("pixels", C.c_int64), ("rel_error", C.c_double), ("abs_rms", C.c_double),
                ("sum_se2", C.c_double), ("sum_mean2", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DisplayParams(C.Structure):
    """mcpt_display_params: exposure, tone curve and transfer of the display transform (all zero: imshow's bytes)"""
    _fields_ = [("exposure", C.c_double), ("auto_key", C.c_double), ("percentile", C.c_double), ("white", C.c_double),
                ("curve", C.c_int32), ("transfer", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class DisplayInfo(C.Structure):
    """mcpt_display_info: what a display call used (exposure, white) and what its histogram held"""
    _fields_ = [("exposure", C.c_double), ("white", C.c_double), ("log_average", C.c_double), ("l_percentile", C.c_double),
                ("counted", C.c_int64), ("skipped", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class QueryParams(C.Structure):
    """mcpt_query_params: samples per query, first sample index, seed, kind and flags of a radiance query"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("kind", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class ShParams(C.Structure):
    """mcpt_sh_params: samples per probe, first sample index, seed and flags of a light-probe call"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("flags", C.c_int32), ("reserved", C.c_int32 * 3)]


class LightmapParams(C.Structure):
    """mcpt_lightmap_params: a lightmap's size, samples per texel, first sample index, seed, flags and dilation rounds"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64),
                ("flags", C.c_int32), ("dilate", C.c_int32), ("reserved", C.c_int32 * 2)]


class LightmapDenoiseParams(C.Structure):
    """mcpt_lightmap_denoise_params: the map's size, the filter's iterations, the dilation rounds and the two sigmas (0: the default)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("dilate", C.c_int32),
                ("sigma_l", C.c_double), ("sigma_p", C.c_double), ("reserved", C.c_int32 * 2)]


class VolumeGrid(C.Structure):
    """mcpt_volume_grid: origin, spacing and probe counts of an irradiance volume's grid, and its flags (api.volume_grid makes one)"""
    _fields_ = [("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 4)]

    @property
    def num_probes(self):
        return self.nx * self.ny * self.nz


class VisibilityParams(C.Structure):
    """mcpt_visibility_params: samples per probe, first sample index, seed, the octahedral map's resolution, the depth clamp, the share of
    back-face hits a valid probe may have, and the workspace's size in rays (0: the default)"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("res", C.c_int32), ("reserved0", C.c_int32),
                ("max_distance", C.c_double), ("max_back_fraction", C.c_double), ("workspace_rays", C.c_int64), ("reserved", C.c_int32 * 2)]


class VolumeVisibility(C.Structure):
    """mcpt_volume_visibility: what the visibility-weighted lookup needs of a bake (res, max_distance) and its own knobs (normal_bias,
    min_visibility); api.volume_visibility makes one"""
    _fields_ = [("res", C.c_int32), ("flags", C.c_int32), ("max_distance", C.c_double), ("normal_bias", C.c_double),
                ("min_visibility", C.c_double), ("reserved", C.c_int32 * 4)]


class BakedSource(C.Structure):
    """mcpt_baked_source: what lights the surfaces of a baked frame -- an irradiance volume (grid, sh27, valid, moments, visibility) or a
    lightmap (uv6, width, height, irradiance3, owner); api.baked_volume and api.baked_lightmap make the Python-side holders"""
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("grid", C.POINTER(VolumeGrid)), ("sh27", C.c_void_p), ("valid", C.c_void_p),
                ("moments", C.c_void_p), ("visibility", C.POINTER(VolumeVisibility)), ("uv6", C.c_void_p), ("width", C.c_int32),
                ("height", C.c_int32), ("irradiance3", C.c_void_p), ("owner", C.c_void_p), ("reserved", C.c_int64 * 4)]


class BakedOutputs(C.Structure):
    """mcpt_baked_outputs: where mcpt_baked_radiance puts its answers, ray by ray; every pointer may be null"""
    _fields_ = [("radiance3", C.c_void_p), ("kind", C.c_void_p), ("face", C.c_void_p), ("q6", C.c_void_p), ("uv2", C.c_void_p),
                ("kd3", C.c_void_p), ("e3", C.c_void_p), ("lit", C.c_void_p), ("reserved", C.c_int64 * 2)]


class BakedFrameParams(C.Structure):
    """mcpt_baked_frame_params: camera samples per pixel, MCPT_BAKED_* flags, seed, and the workspace's size in rays (0: the default)"""
    _fields_ = [("samples", C.c_int32), ("flags", C.c_int32), ("seed", C.c_uint64), ("workspace_rays", C.c_int64), ("reserved", C.c_int32 * 2)]


class ReflectionParams(C.Structure):
    """mcpt_reflection_params: samples per texel, the sample index, seed, the octahedral map's resolution, flags, and the workspace's size
    in rays (0: the default)"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("res", C.c_int32), ("flags", C.c_int32),
                ("workspace_rays", C.c_int64), ("reserved", C.c_int32 * 4)]


class ReflectionChain(C.Structure):
    """mcpt_reflection_chain: the source map's resolution and the resolution and Phong exponent of each of 1 .. 8 prefiltered levels
    (api.reflection_chain makes one)"""
    _fields_ = [("res", C.c_int32), ("num_levels", C.c_int32), ("level_res", C.c_int32 * 8), ("level_ns", C.c_int32 * 8),
                ("reserved", C.c_int32 * 4)]

    @property
    def num_texels(self):
        return sum(self.level_res[l] ** 2 for l in range(max(0, min(self.num_levels, 8))))


class BakedSpecular(C.Structure):
    """mcpt_baked_specular: the reflection volume a baked call adds ks * R from -- grid, chain description, chain data, valid, moments
    and visibility; api.baked_reflection makes the Python-side holder"""
    _fields_ = [("flags", C.c_int32), ("pad", C.c_int32), ("grid", C.POINTER(VolumeGrid)), ("chain", C.POINTER(ReflectionChain)),
                ("chain_data", C.c_void_p), ("valid", C.c_void_p), ("moments", C.c_void_p), ("visibility", C.POINTER(VolumeVisibility)),
                ("reserved", C.c_int64 * 4)]


class BakedSpecularOutputs(C.Structure):
    """mcpt_baked_specular_outputs: where mcpt_baked_radiance_specular puts the specular term's parts, ray by ray; every pointer may be null"""
    _fields_ = [("spec3", C.c_void_p), ("ks3", C.c_void_p), ("r3", C.c_void_p), ("ns", C.c_void_p), ("slit", C.c_void_p),
                ("reserved", C.c_int64 * 2)]


class OcclusionParams(C.Structure):
    """mcpt_occlusion_params: samples per entry, first sample index, seed, the falloff (MCPT_OCCLUSION_*), flags (0), the distance beyond
    which a hit no longer occludes, and the workspace's size in rays (0: the default)"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("falloff", C.c_int32), ("flags", C.c_int32),
                ("max_distance", C.c_double), ("workspace_rays", C.c_int64), ("reserved", C.c_int32 * 2)]


class OcclusionMap(C.Structure):
    """mcpt_occlusion_map: an occlusion map's size and dilation rounds"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("dilate", C.c_int32), ("reserved", C.c_int32)]


class PairParams(C.Structure):
    """mcpt_pair_params: the part [t0, t1] of every segment a -> b that a pair matrix asks about, and flags (0)"""
    _fields_ = [("t0", C.c_double), ("t1", C.c_double), ("flags", C.c_int32), ("reserved", C.c_int32)]


class DirectLight(C.Structure):
    """mcpt_direct_light: one of a caller's own lights -- type (MCPT_LIGHT_*), flags (MCPT_LIGHT_TWO_SIDED on a rectangle), position,
    direction (the way the light travels), the rectangle's edges u and v, colour, a spot's two cosines and a point or spot light's range"""
    _fields_ = [("type", C.c_int32), ("flags", C.c_int32), ("position", C.c_double * 3), ("direction", C.c_double * 3), ("u", C.c_double * 3),
                ("v", C.c_double * 3), ("color", C.c_double * 3), ("cos_inner", C.c_double), ("cos_outer", C.c_double), ("range", C.c_double)]


class DirectParams(C.Structure):
    """mcpt_direct_params: samples per rectangle light, first sample index, seed, the shadow rays' offset along themselves, flags (0)"""
    _fields_ = [("spp", C.c_int32), ("sample_base", C.c_int32), ("seed", C.c_uint64), ("bias", C.c_double), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class DirectMap(C.Structure):
    """mcpt_direct_map: a direct lightmap's size and dilation rounds"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("dilate", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/mcpt.h declares
EXPORTS = [
    "mcpt_version", "mcpt_last_error", "mcpt_device_count", "mcpt_build_id",
    "mcpt_knobs_describe", "mcpt_hip_runtime_info", "mcpt_hip_runtime_check", "mcpt_allow_runtime_mismatch",
    "mcpt_scene_load", "mcpt_scene_load_ex", "mcpt_scene_create", "mcpt_scene_free", "mcpt_scene_set_resolution", "mcpt_scene_get_info", "mcpt_scene_get_faces",
    "mcpt_scene_get_leaf_order", "mcpt_scene_get_bvh_nodes", "mcpt_scene_find_index", "mcpt_scene_get_material",
    "mcpt_scene_get_light", "mcpt_morton_code", "mcpt_scene_fast_bvh_stats",
    "mcpt_device_create", "mcpt_device_create_ex", "mcpt_device_get_bvh_nodes", "mcpt_device_get_leaf_order", "mcpt_device_fast_hierarchy", "mcpt_device_free",
    "mcpt_device_set_trace_mode", "mcpt_scene_trace_engine",
    "mcpt_trace_closest", "mcpt_trace_closest_device",
    "mcpt_render", "mcpt_render_device", "mcpt_device_collect_stats", "mcpt_sample_radiance", "mcpt_owned_pixels",
    "mcpt_quantize_rgb8", "mcpt_write_png", "mcpt_png_encode", "mcpt_png_encode_deflate", "mcpt_write_png_deflate", "mcpt_write_pfm",
    "mcpt_checkpoint_save", "mcpt_checkpoint_load", "mcpt_decode_jpeg",
    "mcpt_progressive_create", "mcpt_progressive_step", "mcpt_progressive_done", "mcpt_progressive_noise", "mcpt_progressive_image",
    "mcpt_progressive_image_device", "mcpt_progressive_next_pass", "mcpt_progressive_free",
    "mcpt_progressive_create_adaptive", "mcpt_progressive_active", "mcpt_progressive_active_pixels", "mcpt_progressive_sample_counts",
    "mcpt_progressive_aovs", "mcpt_progressive_denoise", "mcpt_progressive_denoise_device",
    "mcpt_progressive_sample_aovs", "mcpt_progressive_denoise_guided", "mcpt_progressive_denoise_guided_device",
    "mcpt_multi_create", "mcpt_multi_num_devices", "mcpt_multi_render", "mcpt_multi_render_device", "mcpt_multi_last_timing", "mcpt_multi_collect_stats", "mcpt_multi_free",
    "mcpt_comm_unique_id", "mcpt_comm_create", "mcpt_comm_size", "mcpt_comm_gather_frame", "mcpt_comm_allreduce", "mcpt_comm_free",
    "mcpt_render_scene", "mcpt_render_scene_ex", "mcpt_render_scene_opts",
    "mcpt_device_set_lens", "mcpt_device_get_lens", "mcpt_camera_rays", "mcpt_multi_set_lens", "mcpt_render_scene_lens",
    "mcpt_device_set_environment", "mcpt_device_get_environment", "mcpt_environment_eval", "mcpt_environment_sample", "mcpt_read_pfm",
    "mcpt_multi_set_environment", "mcpt_render_scene_env",
    "mcpt_device_update_vertices", "mcpt_device_update_vertices_device", "mcpt_device_get_vertices", "mcpt_device_set_camera",
    "mcpt_device_get_camera", "mcpt_multi_update_vertices", "mcpt_multi_set_camera",
    "mcpt_device_set_motion", "mcpt_device_set_motion_device", "mcpt_device_clear_motion", "mcpt_device_get_motion", "mcpt_device_motion_info",
    "mcpt_shutter_time", "mcpt_shutter_step", "mcpt_render_scene_motion",
    "mcpt_device_set_light_sampling", "mcpt_device_get_light_sampling", "mcpt_multi_set_light_sampling", "mcpt_scene_light_pick_table",
    "mcpt_light_pick", "mcpt_render_scene_lights",
    "mcpt_scene_light_tree", "mcpt_scene_light_tree_pdf", "mcpt_light_pick_at",
    "mcpt_display_histogram_device", "mcpt_display_histogram", "mcpt_display_exposure", "mcpt_display_device", "mcpt_display",
    "mcpt_display_host", "mcpt_progressive_display", "mcpt_progressive_display_device", "mcpt_render_scene_display",
    "mcpt_query_radiance", "mcpt_query_radiance_device", "mcpt_query_rays",
    "mcpt_query_sh", "mcpt_query_sh_device", "mcpt_query_sh_rays", "mcpt_sh_basis", "mcpt_sh_radiance", "mcpt_sh_irradiance",
    "mcpt_lightmap_raster_host", "mcpt_lightmap_texels", "mcpt_bake_lightmap", "mcpt_bake_lightmap_device",
    "mcpt_query_pass_boundaries", "mcpt_query_radiance_adaptive", "mcpt_query_radiance_adaptive_device",
    "mcpt_bake_lightmap_adaptive", "mcpt_bake_lightmap_adaptive_device",
    "mcpt_lightmap_denoise", "mcpt_lightmap_denoise_device",
    "mcpt_volume_points", "mcpt_bake_volume", "mcpt_bake_volume_device",
    "mcpt_volume_irradiance_host", "mcpt_volume_irradiance", "mcpt_volume_irradiance_device",
    "mcpt_visibility_bin", "mcpt_query_visibility", "mcpt_query_visibility_device",
    "mcpt_bake_volume_visibility", "mcpt_bake_volume_visibility_device",
    "mcpt_volume_irradiance_visible_host", "mcpt_volume_irradiance_visible", "mcpt_volume_irradiance_visible_device",
    "mcpt_lightmap_irradiance_host", "mcpt_lightmap_irradiance", "mcpt_lightmap_irradiance_device",
    "mcpt_baked_radiance", "mcpt_baked_radiance_device", "mcpt_render_baked", "mcpt_render_baked_device",
    "mcpt_reflection_texels", "mcpt_bake_reflection", "mcpt_bake_reflection_device", "mcpt_reflection_rays",
    "mcpt_reflection_prefilter_host", "mcpt_reflection_prefilter", "mcpt_reflection_prefilter_device",
    "mcpt_reflection_lookup_host", "mcpt_reflection_lookup", "mcpt_reflection_lookup_device",
    "mcpt_reflection_volume_lookup_host", "mcpt_reflection_volume_lookup", "mcpt_reflection_volume_lookup_device",
    "mcpt_baked_radiance_specular", "mcpt_baked_radiance_specular_device", "mcpt_render_baked_specular", "mcpt_render_baked_specular_device",
    "mcpt_query_occlusion", "mcpt_query_occlusion_device", "mcpt_occlusion_fold_host",
    "mcpt_bake_occlusion_lightmap", "mcpt_bake_occlusion_lightmap_device",
    "mcpt_trace_any", "mcpt_trace_any_device", "mcpt_pair_rays", "mcpt_trace_any_pairs", "mcpt_trace_any_pairs_device",
    "mcpt_query_direct", "mcpt_query_direct_device", "mcpt_direct_slots", "mcpt_direct_rays", "mcpt_direct_fold_host",
    "mcpt_bake_direct_lightmap", "mcpt_bake_direct_lightmap_device",
]


def build(verbose=False):
    """Compile libmcpt.so in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC, "-j8", "all"], stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libmcpt.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C montecarlopathtracing_amd/csrc` (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    P, D, I32, U8 = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.mcpt_version.restype = C.c_int
    L.mcpt_last_error.restype = C.c_char_p
    L.mcpt_device_count.restype = C.c_int
    L.mcpt_build_id.restype = C.c_char_p
    L.mcpt_knobs_describe.restype = C.c_char_p
    L.mcpt_hip_runtime_info.argtypes = [I32, I32, C.c_char_p, C.c_int64]
    L.mcpt_hip_runtime_check.argtypes = [C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.c_int64]
    L.mcpt_allow_runtime_mismatch.argtypes = [C.c_int32]
    L.mcpt_allow_runtime_mismatch.restype = None
    L.mcpt_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(P)]
    L.mcpt_scene_load_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(P)]
    L.mcpt_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int32, C.POINTER(P)]
    L.mcpt_scene_free.argtypes = [P]
    L.mcpt_scene_free.restype = None
    L.mcpt_scene_set_resolution.argtypes = [P, C.c_int32, C.c_int32]
    L.mcpt_scene_get_info.argtypes = [P, C.POINTER(SceneInfo)]
    L.mcpt_scene_get_faces.argtypes = [P, D, I32, C.POINTER(C.c_uint32)]
    L.mcpt_scene_get_leaf_order.argtypes = [P, I32]
    L.mcpt_scene_get_bvh_nodes.argtypes = [P, D, I32, I32]
    L.mcpt_scene_find_index.argtypes = [P, C.c_int32, C.c_int32]
    L.mcpt_scene_get_material.argtypes = [P, C.c_int32, C.c_char_p, D, I32]
    L.mcpt_scene_get_light.argtypes = [P, C.c_int32, C.c_char_p, D, I32, D]
    L.mcpt_morton_code.restype = C.c_uint32
    L.mcpt_morton_code.argtypes = [C.c_float, C.c_float, C.c_float]
    L.mcpt_scene_fast_bvh_stats.argtypes = [P, I32, I32, I32, I32]
    L.mcpt_device_create.argtypes = [P, C.c_int32, C.POINTER(P)]
    L.mcpt_device_create_ex.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(P)]
    L.mcpt_device_get_bvh_nodes.argtypes = [P, D, I32]
    L.mcpt_device_get_leaf_order.argtypes = [P, I32]
    L.mcpt_device_fast_hierarchy.argtypes = [P, C.POINTER(FastInfo), P, I32]
    L.mcpt_device_free.argtypes = [P]
    L.mcpt_device_free.restype = None
    L.mcpt_device_set_trace_mode.argtypes = [P, C.c_int32]
    L.mcpt_scene_trace_engine.argtypes = [P]
    L.mcpt_trace_closest.argtypes = [P, D, C.c_int64, I32, D, D, D, C.POINTER(Stats)]
    L.mcpt_trace_closest_device.argtypes = [P, P, C.c_int64, P, P, P, P, P]
    L.mcpt_render.argtypes = [P, C.POINTER(RenderParams), D, C.POINTER(Stats)]
    L.mcpt_render_device.argtypes = [P, C.POINTER(RenderParams), P, C.POINTER(Stats), P]
    L.mcpt_device_collect_stats.argtypes = [P, C.POINTER(Stats)]
    L.mcpt_sample_radiance.argtypes = [P, C.c_uint64, I32, I32, C.c_int64, D]
    L.mcpt_owned_pixels.restype = C.c_int64
    L.mcpt_owned_pixels.argtypes = [P, C.POINTER(RenderParams), I32]
    L.mcpt_quantize_rgb8.argtypes = [D, C.c_int64, U8]
    L.mcpt_write_png.argtypes = [C.c_char_p, U8, C.c_int32, C.c_int32]
    L.mcpt_png_encode.restype = C.c_int64
    L.mcpt_png_encode.argtypes = [U8, C.c_int32, C.c_int32, U8, C.c_int64]
    L.mcpt_png_encode_deflate.restype = C.c_int64
    L.mcpt_png_encode_deflate.argtypes = [U8, C.c_int32, C.c_int32, U8, C.c_int64]
    L.mcpt_write_png_deflate.argtypes = [C.c_char_p, U8, C.c_int32, C.c_int32]
    L.mcpt_write_pfm.argtypes = [C.c_char_p, D, C.c_int32, C.c_int32]
    L.mcpt_checkpoint_save.argtypes = [C.c_char_p, P, D, C.c_int32, C.c_uint64, C.c_int32, U8]
    L.mcpt_checkpoint_load.argtypes = [C.c_char_p, P, D, C.c_int32, C.c_uint64, C.c_int32, U8]
    L.mcpt_decode_jpeg.argtypes = [C.c_char_p, I32, I32, U8, C.c_int64]
    L.mcpt_progressive_create.argtypes = [P, C.POINTER(RenderParams), C.POINTER(P)]
    L.mcpt_progressive_step.argtypes = [P, C.c_int32, C.POINTER(Stats)]
    L.mcpt_progressive_done.argtypes = [P]
    L.mcpt_progressive_noise.argtypes = [P, C.POINTER(Noise)]
    L.mcpt_progressive_image.argtypes = [P, D, D]
    L.mcpt_progressive_image_device.argtypes = [P, P, P, P]
    L.mcpt_progressive_next_pass.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double]
    L.mcpt_progressive_free.argtypes = [P]
    L.mcpt_progressive_free.restype = None
    L.mcpt_progressive_create_adaptive.argtypes = [P, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), C.POINTER(P)]
    L.mcpt_progressive_active.argtypes = [P]
    L.mcpt_progressive_active.restype = C.c_int64
    L.mcpt_progressive_active_pixels.argtypes = [P, I32]
    L.mcpt_progressive_active_pixels.restype = C.c_int64
    L.mcpt_progressive_sample_counts.argtypes = [P, I32]
    L.mcpt_progressive_aovs.argtypes = [P, I32, D, D, D]
    L.mcpt_progressive_denoise.argtypes = [P, C.POINTER(DenoiseParams), D]
    L.mcpt_progressive_denoise_device.argtypes = [P, C.POINTER(DenoiseParams), P, P]
    L.mcpt_progressive_sample_aovs.argtypes = [P, C.c_int32, I32, D, D, D]
    L.mcpt_progressive_denoise_guided.argtypes = [P, C.POINTER(DenoiseParams), C.POINTER(GuideParams), D]
    L.mcpt_progressive_denoise_guided_device.argtypes = [P, C.POINTER(DenoiseParams), C.POINTER(GuideParams), P, P]
    L.mcpt_multi_create.argtypes = [P, I32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(P)]
    L.mcpt_multi_num_devices.argtypes = [P]
    L.mcpt_multi_render.argtypes = [P, C.POINTER(RenderParams), D, C.POINTER(Stats)]
    L.mcpt_multi_render_device.argtypes = [P, C.POINTER(RenderParams), C.POINTER(P), C.POINTER(Stats)]
    L.mcpt_multi_last_timing.argtypes = [P, D, D, I32]
    L.mcpt_multi_collect_stats.argtypes = [P, C.POINTER(Stats)]
    L.mcpt_multi_free.argtypes = [P]
    L.mcpt_multi_free.restype = None
    L.mcpt_comm_unique_id.argtypes = [U8, C.c_int64]
    L.mcpt_comm_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, U8, C.c_int64, C.POINTER(P)]
    L.mcpt_comm_size.argtypes = [P]
    L.mcpt_comm_gather_frame.argtypes = [P, P, C.POINTER(RenderParams), P, P]
    L.mcpt_comm_allreduce.argtypes = [P, D, C.c_int32, C.c_int32]
    L.mcpt_comm_free.argtypes = [P]
    L.mcpt_comm_free.restype = None
    L.mcpt_render_scene.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
    L.mcpt_render_scene_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.POINTER(Stats)]
    L.mcpt_render_scene_opts.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Stats)]
    L.mcpt_device_set_lens.argtypes = [P, C.POINTER(Lens)]
    L.mcpt_device_get_lens.argtypes = [P, C.POINTER(Lens)]
    L.mcpt_camera_rays.argtypes = [P, C.c_uint64, I32, I32, C.c_int64, D]
    L.mcpt_multi_set_lens.argtypes = [P, C.POINTER(Lens)]
    L.mcpt_render_scene_lens.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Lens),
                                         C.POINTER(Stats)]
    F32 = C.POINTER(C.c_float)
    L.mcpt_device_set_environment.argtypes = [P, C.POINTER(Environment)]
    L.mcpt_device_get_environment.argtypes = [P, I32, I32, D, D]
    L.mcpt_environment_eval.argtypes = [P, D, C.c_int64, D]
    L.mcpt_environment_sample.argtypes = [P, C.c_uint64, I32, I32, C.c_int32, C.c_int64, D, D, D]
    L.mcpt_read_pfm.argtypes = [C.c_char_p, I32, I32, F32, C.c_int64]
    L.mcpt_multi_set_environment.argtypes = [P, C.POINTER(Environment)]
    L.mcpt_render_scene_env.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Lens), C.c_char_p,
                                        C.c_double, C.POINTER(Stats)]
    L.mcpt_device_update_vertices.argtypes = [P, D, C.c_int32, C.POINTER(UpdateInfo)]
    L.mcpt_device_update_vertices_device.argtypes = [P, P, C.c_int32, C.POINTER(UpdateInfo), P]
    L.mcpt_device_get_vertices.argtypes = [P, D]
    L.mcpt_device_set_camera.argtypes = [P, D, D, D, C.c_double]
    L.mcpt_device_get_camera.argtypes = [P, D, D, D, D]
    L.mcpt_multi_update_vertices.argtypes = [P, D, C.c_int32, C.POINTER(UpdateInfo)]
    L.mcpt_multi_set_camera.argtypes = [P, D, D, D, C.c_double]
    L.mcpt_device_set_motion.argtypes = [P, D, C.POINTER(CameraKey), C.POINTER(Shutter)]
    L.mcpt_device_set_motion_device.argtypes = [P, P, C.POINTER(CameraKey), C.POINTER(Shutter), P]
    L.mcpt_device_clear_motion.argtypes = [P]
    L.mcpt_device_get_motion.argtypes = [P, C.POINTER(Shutter), I32, I32, C.POINTER(CameraKey)]
    L.mcpt_device_motion_info.argtypes = [P, C.POINTER(MotionInfo)]
    L.mcpt_shutter_time.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_int32]
    L.mcpt_shutter_time.restype = C.c_double
    L.mcpt_shutter_step.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.mcpt_shutter_step.restype = C.c_int32
    L.mcpt_render_scene_motion.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Lens), C.c_char_p,
                                           C.c_double, C.c_char_p, C.c_char_p, C.POINTER(Shutter), C.POINTER(Stats)]
    L.mcpt_device_set_light_sampling.argtypes = [P, C.POINTER(LightSampling)]
    L.mcpt_device_get_light_sampling.argtypes = [P, I32, D]
    L.mcpt_multi_set_light_sampling.argtypes = [P, C.POINTER(LightSampling)]
    L.mcpt_scene_light_pick_table.argtypes = [P, D, D, D]
    L.mcpt_light_pick.argtypes = [P, C.c_uint64, I32, I32, C.c_int32, C.c_int64, I32, D]
    L.mcpt_scene_light_tree.argtypes = [P, D, I32, C.c_void_p]
    L.mcpt_scene_light_tree_pdf.argtypes = [P, D, D, D, C.c_int64, D]
    L.mcpt_light_pick_at.argtypes = [P, C.c_uint64, I32, I32, C.c_int32, D, D, C.c_int64, I32, D]
    L.mcpt_render_scene_lights.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Lens), C.c_char_p,
                                           C.c_double, C.POINTER(LightSampling), C.POINTER(Stats)]
    I64 = C.POINTER(C.c_int64)
    DP, DI = C.POINTER(DisplayParams), C.POINTER(DisplayInfo)
    L.mcpt_display_histogram_device.argtypes = [P, P, C.c_int64, I64, P]
    L.mcpt_display_histogram.argtypes = [P, D, C.c_int64, I64]
    L.mcpt_display_exposure.argtypes = [I64, C.c_double, D, D]
    L.mcpt_display_device.argtypes = [P, P, C.c_int64, DP, P, DI, P]
    L.mcpt_display.argtypes = [P, D, C.c_int64, DP, U8, DI]
    L.mcpt_display_host.argtypes = [D, C.c_int64, DP, U8, DI]
    L.mcpt_progressive_display.argtypes = [P, C.c_int32, DP, U8, DI]
    L.mcpt_progressive_display_device.argtypes = [P, C.c_int32, DP, P, DI, P]
    L.mcpt_render_scene_display.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(RenderSceneOptions), C.c_int64, C.POINTER(Lens), C.c_char_p,
                                            C.c_double, C.POINTER(LightSampling), DP, C.POINTER(Stats)]
    QP = C.POINTER(QueryParams)
    L.mcpt_query_radiance.argtypes = [P, D, I32, C.c_int64, QP, D, D, I32, C.POINTER(Stats)]
    L.mcpt_query_radiance_device.argtypes = [P, P, P, C.c_int64, QP, P, P, P, C.POINTER(Stats), P]
    L.mcpt_query_rays.argtypes = [P, D, I32, C.c_int64, C.c_uint64, C.c_int32, I32, D]
    SP = C.POINTER(ShParams)
    L.mcpt_query_sh.argtypes = [P, D, I32, C.c_int64, SP, D, D, I32, C.POINTER(Stats)]
    L.mcpt_query_sh_device.argtypes = [P, P, P, C.c_int64, SP, P, P, P, C.POINTER(Stats), P]
    L.mcpt_query_sh_rays.argtypes = [P, D, I32, C.c_int64, C.c_uint64, I32, D]
    L.mcpt_sh_basis.argtypes = [D, C.c_int64, D]
    L.mcpt_sh_radiance.argtypes = [D, D, C.c_int64, D]
    L.mcpt_sh_irradiance.argtypes = [D, D, C.c_int64, D]
    LP = C.POINTER(LightmapParams)
    L.mcpt_lightmap_raster_host.argtypes = [D, C.c_int64, C.c_int32, C.c_int32, I32]
    L.mcpt_lightmap_texels.argtypes = [P, D, C.c_int32, C.c_int32, I32, I32, D, C.c_int64]
    L.mcpt_lightmap_texels.restype = C.c_int64
    L.mcpt_bake_lightmap.argtypes = [P, D, LP, D, D, I32, I32, C.POINTER(Stats)]
    L.mcpt_bake_lightmap_device.argtypes = [P, P, LP, P, P, P, P, C.POINTER(Stats), P]
    AP = C.POINTER(AdaptiveParams)
    L.mcpt_query_pass_boundaries.argtypes = [C.c_int32, C.c_int32, I32, C.c_int32]
    L.mcpt_query_radiance_adaptive.argtypes = [P, D, I32, C.c_int64, QP, AP, D, D, I32, I32, C.POINTER(Stats)]
    L.mcpt_query_radiance_adaptive_device.argtypes = [P, P, P, C.c_int64, QP, AP, P, P, P, P, C.POINTER(Stats), P]
    L.mcpt_bake_lightmap_adaptive.argtypes = [P, D, LP, AP, D, D, I32, I32, I32, C.POINTER(Stats)]
    L.mcpt_bake_lightmap_adaptive_device.argtypes = [P, P, LP, AP, P, P, P, P, P, C.POINTER(Stats), P]
    LDP = C.POINTER(LightmapDenoiseParams)
    L.mcpt_lightmap_denoise.argtypes = [P, D, LDP, D, D, D, I32]
    L.mcpt_lightmap_denoise_device.argtypes = [P, P, LDP, P, P, P, P, P]
    VG = C.POINTER(VolumeGrid)
    L.mcpt_volume_points.argtypes = [VG, D]
    L.mcpt_bake_volume.argtypes = [P, VG, SP, D, D, I32, C.POINTER(Stats)]
    L.mcpt_bake_volume_device.argtypes = [P, VG, SP, P, P, P, C.POINTER(Stats), P]
    L.mcpt_volume_irradiance_host.argtypes = [VG, D, U8, D, C.c_int64, D, I32]
    L.mcpt_volume_irradiance.argtypes = [P, VG, D, U8, D, C.c_int64, D, I32]
    L.mcpt_volume_irradiance_device.argtypes = [P, VG, P, P, P, C.c_int64, P, P, P]
    VP, VV = C.POINTER(VisibilityParams), C.POINTER(VolumeVisibility)
    L.mcpt_visibility_bin.argtypes = [D, C.c_int64, C.c_int32, I32]
    L.mcpt_query_visibility.argtypes = [P, D, I32, C.c_int64, VP, D, I32, I32, U8, C.POINTER(Stats)]
    L.mcpt_query_visibility_device.argtypes = [P, P, P, C.c_int64, VP, P, P, P, P, C.POINTER(Stats), P]
    L.mcpt_bake_volume_visibility.argtypes = [P, VG, VP, D, I32, I32, U8, C.POINTER(Stats)]
    L.mcpt_bake_volume_visibility_device.argtypes = [P, VG, VP, P, P, P, P, C.POINTER(Stats), P]
    L.mcpt_volume_irradiance_visible_host.argtypes = [VG, D, D, U8, VV, D, C.c_int64, D, I32]
    L.mcpt_volume_irradiance_visible.argtypes = [P, VG, D, D, U8, VV, D, C.c_int64, D, I32]
    L.mcpt_volume_irradiance_visible_device.argtypes = [P, VG, P, P, P, VV, P, C.c_int64, P, P, P]
    BS, BO, BF = C.POINTER(BakedSource), C.POINTER(BakedOutputs), C.POINTER(BakedFrameParams)
    L.mcpt_lightmap_irradiance_host.argtypes = [C.c_int32, C.c_int32, D, I32, D, C.c_int64, D, I32]
    L.mcpt_lightmap_irradiance.argtypes = [P, C.c_int32, C.c_int32, D, I32, D, C.c_int64, D, I32]
    L.mcpt_lightmap_irradiance_device.argtypes = [P, C.c_int32, C.c_int32, P, P, P, C.c_int64, P, P, P]
    L.mcpt_baked_radiance.argtypes = [P, BS, D, C.c_int64, C.c_int32, BO, C.POINTER(Stats)]
    L.mcpt_baked_radiance_device.argtypes = [P, BS, P, C.c_int64, C.c_int32, BO, C.POINTER(Stats), P]
    L.mcpt_render_baked.argtypes = [P, BS, BF, D, I32, I32, C.POINTER(Stats)]
    L.mcpt_render_baked_device.argtypes = [P, BS, BF, P, P, P, C.POINTER(Stats), P]
    RP, RC = C.POINTER(ReflectionParams), C.POINTER(ReflectionChain)
    L.mcpt_reflection_texels.argtypes = [C.c_int32, D, D]
    L.mcpt_bake_reflection.argtypes = [P, D, I32, C.c_int64, RP, D, D, I32, C.POINTER(Stats)]
    L.mcpt_bake_reflection_device.argtypes = [P, P, P, C.c_int64, RP, P, P, P, C.POINTER(Stats), P]
    L.mcpt_reflection_rays.argtypes = [P, D, I32, C.c_int64, RP, I64, C.c_int64, D, I32]
    L.mcpt_reflection_prefilter_host.argtypes = [RC, D, C.c_int64, D]
    L.mcpt_reflection_prefilter.argtypes = [P, RC, D, C.c_int64, D]
    L.mcpt_reflection_prefilter_device.argtypes = [P, RC, P, C.c_int64, P, P]
    L.mcpt_reflection_lookup_host.argtypes = [RC, D, C.c_int64, I32, D, D, C.c_int64, D]
    L.mcpt_reflection_lookup.argtypes = [P, RC, D, C.c_int64, I32, D, D, C.c_int64, D]
    L.mcpt_reflection_lookup_device.argtypes = [P, RC, P, C.c_int64, P, P, P, C.c_int64, P, P]
    VG, VV = C.POINTER(VolumeGrid), C.POINTER(VolumeVisibility)
    SP, SO = C.POINTER(BakedSpecular), C.POINTER(BakedSpecularOutputs)
    L.mcpt_reflection_volume_lookup_host.argtypes = [VG, RC, D, U8, D, VV, D, D, D, C.c_int64, D, I32]
    L.mcpt_reflection_volume_lookup.argtypes = [P, VG, RC, D, U8, D, VV, D, D, D, C.c_int64, D, I32]
    L.mcpt_reflection_volume_lookup_device.argtypes = [P, VG, RC, P, P, P, VV, P, P, P, C.c_int64, P, P, P]
    L.mcpt_baked_radiance_specular.argtypes = [P, BS, SP, D, C.c_int64, C.c_int32, BO, SO, C.POINTER(Stats)]
    L.mcpt_baked_radiance_specular_device.argtypes = [P, BS, SP, P, C.c_int64, C.c_int32, BO, SO, C.POINTER(Stats), P]
    L.mcpt_render_baked_specular.argtypes = [P, BS, SP, BF, D, I32, I32, I32, C.POINTER(Stats)]
    L.mcpt_render_baked_specular_device.argtypes = [P, BS, SP, BF, P, P, P, P, C.POINTER(Stats), P]
    OP, OM = C.POINTER(OcclusionParams), C.POINTER(OcclusionMap)
    L.mcpt_query_occlusion.argtypes = [P, D, I32, C.c_int64, OP, D, D, D, I32, I32, C.POINTER(Stats)]
    L.mcpt_query_occlusion_device.argtypes = [P, P, P, C.c_int64, OP, P, P, P, P, P, C.POINTER(Stats), P]
    L.mcpt_occlusion_fold_host.argtypes = [D, D, I32, D, D, C.c_int64, OP, D, D, D, I32, I32]
    L.mcpt_bake_occlusion_lightmap.argtypes = [P, D, OM, OP, D, D, D, I32, I32, I32, C.POINTER(Stats)]
    L.mcpt_bake_occlusion_lightmap_device.argtypes = [P, P, OM, OP, P, P, P, P, P, P, C.POINTER(Stats), P]
    PP, U8, U64 = C.POINTER(PairParams), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    L.mcpt_trace_any.argtypes = [P, D, D, C.c_int64, U8, C.POINTER(Stats)]
    L.mcpt_trace_any_device.argtypes = [P, P, P, C.c_int64, P, P]
    L.mcpt_pair_rays.argtypes = [D, C.c_int64, D, C.c_int64, PP, D, D]
    L.mcpt_trace_any_pairs.argtypes = [P, D, C.c_int64, D, C.c_int64, PP, U64, C.POINTER(Stats)]
    L.mcpt_trace_any_pairs_device.argtypes = [P, P, C.c_int64, P, C.c_int64, PP, P, P]
    DL, DP, DM = C.POINTER(DirectLight), C.POINTER(DirectParams), C.POINTER(DirectMap)
    L.mcpt_query_direct.argtypes = [P, D, I32, C.c_int64, DL, C.c_int32, DP, D, D, D, D, C.POINTER(Stats)]
    L.mcpt_query_direct_device.argtypes = [P, P, P, C.c_int64, DL, C.c_int32, DP, P, P, P, P, P]
    L.mcpt_direct_slots.argtypes = [DL, C.c_int32, C.c_int32]
    L.mcpt_direct_slots.restype = C.c_int64
    L.mcpt_direct_rays.argtypes = [P, D, I32, C.c_int64, DL, C.c_int32, DP, D, D, D]
    L.mcpt_direct_fold_host.argtypes = [DL, C.c_int32, DP, D, U8, C.c_int64, D, D, D, D]
    L.mcpt_bake_direct_lightmap.argtypes = [P, D, DM, DL, C.c_int32, DP, D, D, D, D, I32, C.POINTER(Stats)]
    L.mcpt_bake_direct_lightmap_device.argtypes = [P, P, DM, DL, C.c_int32, DP, P, P, P, P, P, C.POINTER(Stats), P]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise McptError(rc, lib().mcpt_last_error().decode(errors="replace"))
