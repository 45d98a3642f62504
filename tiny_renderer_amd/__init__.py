"""tiny_renderer_amd -- MI355X-native triangle-fill path of tiny_renderer behind a C ABI.

The product is the shared library built from csrc/ (HIP kernels for gfx950 + C++ host) whose
entry points are declared in include/tiny_renderer.h.  This package is the thin Python mirror
of the reference's `Scene` interface (src/scene.rs:44-269) over that library, used by the
tests, the bench and the headless CLI.  There is no CPU rendering path: creating a Scene
without the built library or without a GPU raises.
"""
from ._lib import build_library, library_path, load_library, TinyRendererError  # noqa: F401
from .scene import Scene, PIPELINES, prepare_uniforms, band_rows, transform_mesh, morph_mesh, morph_deltas, skin_mesh, composite_host, shadow_merge_host, ambient_occlusion_host, ao_offsets, accumulate_host, depth_of_field_host, dof_coc, dof_params, DofParams, bloom_host, bloom_params, BloomParams, grade_host, lut_identity, lut_from_function, load_cube, aa_host, aa_params, AaParams, resize_host, resize_taps, resize_params, ResizeParams, yuv_host, yuv_params, yuv_bytes, yuv_planes, yuv_coefficients, YuvParams, Y4MWriter, layer_host, layer_params, LayerParams, layer_gradient, layer_vignette, layer_checker, layer_letterbox, warp_host, warp_params, WarpParams, warp_grid_shape, warp_grid_identity, warp_grid_from_function, warp_grid_rotate, warp_grid_lens, warp_grid_homography, warp_grid_chromatic, convolve_host, convolve_params, ConvolveParams, kernel_gaussian, kernel_box, kernel_tent, kernel_sobel, kernel_laplacian, kernel_emboss, kernel_motion, outline_host, outline_kinds, outline_params, OutlineParams, texel_set_host, frame_stats_host, frame_stats_merge, hist_percentile, lut_auto_levels, depth_median, stats_params, StatsParams, FrameStats  # noqa: F401
from .assets import load_assets, load_obj, load_tga, save_tga, save_png  # noqa: F401
from .synthetic import synthetic_scene, instanced_grid, grid_instances, apply_instances  # noqa: F401
from .synthetic import instance_transforms, rotation_instances, apply_instance_transforms  # noqa: F401
from .sharded import ShardedScene, PeerExchange, launch_ranks  # noqa: F401

__all__ = ["Scene", "PIPELINES", "prepare_uniforms", "band_rows", "load_assets", "load_obj", "load_tga", "save_tga", "save_png",
           "synthetic_scene", "instanced_grid", "grid_instances", "apply_instances", "instance_transforms",
           "rotation_instances", "apply_instance_transforms", "transform_mesh", "morph_mesh", "morph_deltas", "skin_mesh", "composite_host", "shadow_merge_host", "ambient_occlusion_host", "ao_offsets", "accumulate_host", "depth_of_field_host", "dof_coc", "dof_params", "DofParams", "bloom_host", "bloom_params", "BloomParams", "grade_host", "lut_identity", "lut_from_function", "load_cube", "aa_host", "aa_params", "AaParams", "resize_host", "resize_taps", "resize_params", "ResizeParams", "yuv_host", "yuv_params", "yuv_bytes", "yuv_planes", "yuv_coefficients", "YuvParams", "Y4MWriter", "layer_host", "layer_params", "LayerParams", "layer_gradient", "layer_vignette", "layer_checker", "layer_letterbox", "warp_host", "warp_params", "WarpParams", "warp_grid_shape", "warp_grid_identity", "warp_grid_from_function", "warp_grid_rotate", "warp_grid_lens", "warp_grid_homography", "warp_grid_chromatic", "convolve_host", "convolve_params", "ConvolveParams", "kernel_gaussian", "kernel_box", "kernel_tent", "kernel_sobel", "kernel_laplacian", "kernel_emboss", "kernel_motion", "outline_host", "outline_kinds", "outline_params", "OutlineParams", "texel_set_host", "frame_stats_host", "frame_stats_merge", "hist_percentile", "lut_auto_levels", "depth_median", "stats_params", "StatsParams", "FrameStats", "build_library", "library_path", "load_library",
           "TinyRendererError"]
