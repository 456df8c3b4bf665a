"""MI355X-native Monte-Carlo path tracer behind the surface of Arieys/MonteCarloPathTracing's render_scene.

The work is done by csrc/libmcpt.so (host C++ + hand-written HIP kernels for gfx950, C ABI in include/mcpt.h);
this package is the ctypes face of that ABI plus the one-process-per-GPU tile partition / RCCL gather driver."""
from ._lib import AdaptiveParams, CameraKey, MotionInfo, Shutter, DenoiseParams, DisplayInfo, DisplayParams, GuideParams, Environment, FastInfo, Lens, LightSampling, McptError, Noise, QueryParams, ShParams, LightmapParams, LightmapDenoiseParams, VolumeGrid, VisibilityParams, VolumeVisibility, BakedSource, BakedOutputs, BakedFrameParams, BakedSpecular, BakedSpecularOutputs, ReflectionParams, ReflectionChain, OcclusionParams, OcclusionMap, PairParams, DirectLight, DirectParams, DirectMap, RenderParams, Stats, UpdateInfo, build, lib  # noqa: F401
from .api import (UPDATE_REFIT, UPDATE_REBUILD, FAST_BUILT_DEVICE_FAST, FAST_BUILT_DEVICE_PLOC, FAST_BUILT_HOST, FAST_BUILT_PLOC_FELL_BACK, GATHER_PEER, GATHER_RCCL, LENS_JITTER, LENS_PER_SAMPLE, MultiDevice, BUILD_DEVICE, BUILD_DEVICE_FAST, BUILD_DEVICE_SAH, BUILD_HOST, LOAD_MORTON_BOUNDS, LOAD_MTLLIB, LOAD_STANDARD_OBJ, OUT_AOV_PFM, OUT_DENOISED, OUT_DENOISED_SAMPLES, OUT_SAMPLE_AOV_PFM, OUT_ERROR_PFM, OUT_PFM, OUT_PNG_DEFLATE, OUT_SPP_PFM, Progressive, progressive_next_pass, checkpoint_load, checkpoint_save, png_bytes_deflate, write_pfm, RENDER_DEFAULT, RENDER_MEGAKERNEL, RENDER_KEEP_STATS, RENDER_PIPELINE, TRACE_FAST, TRACE_REFERENCE, Device, Scene, build_id, decode_jpeg, device_count, hip_runtime_path, hip_runtime_info, hip_runtime_check, allow_runtime_mismatch, imshow_rgb8, morton_code, png_bytes, render_scene,  # noqa: F401
                  make_environment, make_lens, make_light_sampling, LIGHTS_ALL, LIGHTS_ONE, LIGHTS_TREE, LIGHT_NODE, read_pfm, write_png, shutter_step, shutter_time,
                  make_display, display_host, display_exposure, CURVE_CLAMP, CURVE_REINHARD, CURVE_FILMIC, TRANSFER_LINEAR, TRANSFER_SRGB,
                  DISPLAY_RGBA, DISPLAY_BINS, DISPLAY_SLOTS, DISPLAY_ESTIMATE, DISPLAY_DENOISED, DISPLAY_DENOISED_GUIDED,
                  QUERY_RAY, QUERY_HEMISPHERE, sh_basis, sh_radiance, sh_irradiance, lightmap_raster, grid_atlas, query_pass_boundaries,
                  LIGHTMAP_DENOISE_ITERATIONS, LIGHTMAP_DENOISE_MAX_ITERATIONS, LIGHTMAP_DENOISE_SIGMA_L, LIGHTMAP_DENOISE_SIGMA_P,
                  VOLUME_CLAMP_ZERO, volume_grid, volume_points, volume_irradiance_host,
                  visibility_bin, volume_visibility, volume_irradiance_visible_host,
                  BAKED_VOLUME, BAKED_LIGHTMAP, BAKED_MISS, BAKED_EMITTER, BAKED_SURFACE, BAKED_FACE_VIEWER, BAKED_LIGHTING_ONLY,
                  lightmap_irradiance_host, baked_volume, baked_lightmap,
                  reflection_chain, reflection_texels, reflection_prefilter_host, reflection_lookup_host,
                  baked_reflection, reflection_volume_lookup_host,
                  OCCLUSION_HARD, OCCLUSION_LINEAR, OCCLUSION_SQUARE, occlusion_fold_host, pair_rays,
                  LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL, LIGHT_RECT, LIGHT_TWO_SIDED, point_light, spot_light, directional_light,
                  rect_light, direct_slots, direct_fold_host)
