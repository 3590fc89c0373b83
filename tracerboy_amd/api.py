"""Host-side mirror of the reference's `class TracerBoy` over the C ABI of libtracerboy_hip.so.

Method names follow /root/reference/TracerBoy/TracerBoy.h:158-398 (LoadScene, Render,
GetDefaultOutputSettings, GetNumberOfSamplesSinceLastInvalidate, Get/SetMaterial, SelectPixel ...).
Everything that produces pixels goes through the HIP library; there is no Python or CPU fallback:
constructing `TracerBoy` without the built extension or without a GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ctypes_abi as abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TB_LIB", os.path.join(_HERE, "libtracerboy_hip.so"))  # TB_LIB: an experimental build of the same library

_lib = None


class TracerBoyError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("tracerboy_hip error %d: %s" % (code, message))
        self.code = code


def lib():
    """Load libtracerboy_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libtracerboy_hip.so is not built: run `python -m tracerboy_amd.build` "
                          "(or __graft_entry__.build()); there is no non-HIP fallback")
    try:
        # PyTorch-ROCm bundles its own libamdhip64; importing it first makes this library bind to the SAME
        # HIP runtime instance, so torch tensors (device memory, RCCL buffers) and tb_* calls can share a process.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    vp = C.c_void_p
    sig = {
        "tb_create": (C.c_int, [P(vp), C.c_int]),
        "tb_create_multi": (C.c_int, [P(vp), P(C.c_int), C.c_int]),
        "tb_group_size": (C.c_int, [vp]),
        "tb_destroy": (None, [vp]),
        "tb_last_error": (C.c_char_p, [vp]),
        "tb_load_scene": (C.c_int, [vp, C.c_char_p]),
        "tb_load_procedural": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
        "tb_scene_info_get": (C.c_int, [vp, P(abi.tb_scene_info)]),
        "tb_default_output_settings": (None, [P(abi.tb_output_settings)]),
        "tb_get_camera": (C.c_int, [vp, P(abi.tb_camera)]),
        "tb_set_camera": (C.c_int, [vp, P(abi.tb_camera)]),
        "tb_get_material": (C.c_int, [vp, C.c_int, P(abi.TbMaterial)]),
        "tb_set_material": (C.c_int, [vp, C.c_int, P(abi.TbMaterial)]),
        "tb_material_count": (C.c_int, [vp]),
        "tb_render": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, P(abi.tb_output_settings), C.c_float]),
        "tb_render_async": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, P(abi.tb_output_settings), C.c_float]),
        "tb_sync": (C.c_int, [vp]),
        "tb_read_accum": (C.c_int, [vp, vp, vp]),
        "tb_default_post_settings": (None, [P(abi.tb_post_settings)]),
        "tb_default_denoiser_settings": (None, [P(abi.tb_denoiser_settings)]),
        "tb_render_realtime": (C.c_int, [vp, C.c_uint32, C.c_uint32, P(abi.tb_output_settings), P(abi.tb_denoiser_settings), C.c_float]),
        "tb_read_realtime": (C.c_int, [vp, C.c_int, vp]),
        "tb_denoise": (C.c_int, [vp, P(abi.tb_denoiser_settings), vp]),
        "tb_read_denoise_stage": (C.c_int, [vp, C.c_int, vp]),
        "tb_render_guides": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "tb_read_guide": (C.c_int, [vp, C.c_int, vp]),
        "tb_set_sample_budget": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "tb_read_sample_budget": (C.c_int, [vp, vp]),
        "tb_budget_stop_converged": (C.c_int, [vp, C.c_float, C.c_uint32, P(C.c_uint64), P(C.c_uint64)]),
        "tb_run_budget_stop": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_float, C.c_uint32, C.c_uint32, P(C.c_uint64), P(C.c_uint64)]),
        "tb_post_process": (C.c_int, [vp, P(abi.tb_post_settings), C.c_uint32, vp, vp]),
        "tb_read_averaged_luminance": (C.c_int, [vp, P(C.c_float)]),
        "tb_write_image_rgba8": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, vp]),
        "tb_write_image_f32": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, vp]),
        "tb_decode_image": (C.c_int, [C.c_char_p, P(C.c_uint32), P(C.c_uint32), P(C.c_int), P(C.c_int), vp]),
        "tb_read_aov": (C.c_int, [vp, C.c_int, vp]),
        "tb_accum_device_ptr": (C.c_int, [vp, P(vp), P(vp)]),
        "tb_read_stats": (C.c_int, [vp, P(abi.tb_readback_stats)]),
        "tb_read_wave_profile": (C.c_int, [vp, P(C.c_uint64)]),
        "tb_read_split_profile": (C.c_int, [vp, P(C.c_uint64)]),
        "tb_plan_defaults": (None, [P(abi.tb_plan_input)]),
        "tb_plan_launch": (C.c_int, [P(abi.tb_plan_input), P(abi.tb_launch_plan)]),
        "tb_variant_waves_hi": (C.c_int, [C.c_char_p]),
        "tb_variant_waves_lds": (C.c_int, [C.c_char_p]),
        "tb_invalidate_history": (None, [vp]),
        "tb_samples_rendered": (C.c_uint32, [vp]),
        "tb_select_pixel": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "tb_set_tile_assignment": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "tb_owned_pixels": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
        "tb_pack_owned_device": (C.c_int, [vp, vp]),
        "tb_pack_owned_device_async": (C.c_int, [vp, vp]),
        "tb_stream": (vp, [vp]),
        "tb_unpack_gathered_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
        "tb_unpack_gathered_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(vp), vp]),
        "tb_set_option": (C.c_int, [vp, C.c_char_p, C.c_int64]),
        "tb_get_option": (C.c_int64, [vp, C.c_char_p]),
        "tb_host_scene_view": (C.c_int, [vp, P(abi.TbSceneView)]),
        "tb_make_frame_constants": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, P(abi.tb_output_settings), C.c_float, P(abi.TbPerFrameConstants)]),
        "tb_last_render_ms": (C.c_float, [vp]),
        "tb_trace_closest": (C.c_int, [vp, C.c_uint32] + [vp] * 11),
        "tb_device_math": (C.c_int, [vp, C.c_int, C.c_uint32, vp, vp, vp]),
        "tb_run_temporal": (C.c_int, [vp, P(abi.TbTemporalConstants)] + [vp] * 8),
        "tb_run_denoise_pass": (C.c_int, [vp, P(abi.TbDenoiserConstants)] + [vp] * 5),
        "tb_run_composite": (C.c_int, [vp, C.c_uint32, C.c_uint32] + [vp] * 4),
        "tb_fsr_constants": (C.c_int, [C.c_uint32] * 4 + [C.c_float, P(abi.TbFsrConstants)]),
        "tb_run_fsr_easu": (C.c_int, [vp, P(abi.TbFsrConstants)] + [C.c_uint32] * 5 + [vp, vp]),
        "tb_run_fsr_rcas": (C.c_int, [vp, P(abi.TbFsrConstants)] + [C.c_uint32] * 3 + [vp, vp]),
        "tb_upscale": (C.c_int, [vp, P(abi.tb_post_settings), C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, vp, vp]),
        "tb_default_visualize_settings": (None, [P(abi.tb_visualize_settings)]),
        "tb_record_paths": (C.c_int, [vp] + [C.c_uint32] * 4 + [vp, P(C.c_uint32)]),
        "tb_clear_paths": (C.c_int, [vp]),
        "tb_read_paths": (C.c_int, [vp, vp, C.c_uint32, P(C.c_uint32)]),
        "tb_visualize_rays": (C.c_int, [vp, P(abi.tb_visualize_settings), vp, vp]),
        "tb_visualize_constants": (C.c_int, [P(abi.tb_camera), C.c_uint32, C.c_uint32, P(abi.tb_visualize_settings), P(abi.TbVisualizeConstants)]),
        "tb_run_visualize_rays": (C.c_int, [vp, P(abi.TbVisualizeConstants), vp, C.c_uint32, vp, vp, vp]),
        "tb_trace_rays": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, vp]),
        "tb_trace_radiance": (C.c_int, [vp, P(abi.tb_output_settings), C.c_float, P(abi.TbRadianceCall), C.c_uint64, vp, vp]),
        "tb_radiance_refusal": (C.c_int, [P(abi.TbRadianceCall), C.c_uint64, vp, vp, C.c_char_p, C.c_uint32]),
        "tb_make_camera_rays": (C.c_int, [vp, P(abi.tb_output_settings), C.c_float] + [C.c_uint32] * 8 + [vp, P(C.c_float)]),
        "tb_bake_lightmap": (C.c_int, [vp, P(abi.tb_output_settings), C.c_float, P(abi.tb_bake_call), vp, vp]),
        "tb_bake_refusal": (C.c_int, [P(abi.tb_bake_call), vp, vp, C.c_char_p, C.c_uint32]),
        "tb_read_bake": (C.c_int, [vp, vp, vp, vp]),
        "tb_run_bake_raster": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, vp, vp, vp]),
        "tb_run_bake_dilate": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]),
        "tb_bake_probes": (C.c_int, [vp, P(abi.tb_output_settings), C.c_float, P(abi.tb_probe_call), vp, vp]),
        "tb_probes_refusal": (C.c_int, [P(abi.tb_probe_call), vp, vp, C.c_char_p, C.c_uint32]),
        "tb_read_probe_maps": (C.c_int, [vp, vp, vp]),
        "tb_sample_probes": (C.c_int, [vp, C.c_uint32, P(abi.tb_probe_grid), C.c_uint32, C.c_float, vp, C.c_uint64, vp, vp, vp]),
        "tb_sh9_irradiance": (C.c_int, [vp, vp, vp]),
        "tb_probe_directions": (C.c_int, [C.c_uint32, vp, vp]),
        "tb_run_probe_rays": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
        "tb_run_probe_project": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
        "tb_nearest_points": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, vp]),
        "tb_bake_distance_field": (C.c_int, [vp, C.c_uint32, P(abi.tb_probe_grid), C.c_float, vp]),
        "tb_nearest_refusal": (C.c_int, [C.c_uint32, C.c_uint64, vp, vp, P(abi.tb_probe_grid), C.c_char_p, C.c_uint32]),
        "tb_host_scene_nearest": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, vp]),
        "tb_host_scene_nearest_excess": (C.c_int, [vp, C.c_uint64, vp, P(C.c_float)]),
        "tb_winding_numbers": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, C.c_float, vp]),
        "tb_bake_winding_field": (C.c_int, [vp, C.c_uint32, P(abi.tb_probe_grid), C.c_float, vp]),
        "tb_nearest_points_winding": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, C.c_float, vp]),
        "tb_bake_distance_field_winding": (C.c_int, [vp, C.c_uint32, P(abi.tb_probe_grid), C.c_float, C.c_float, vp]),
        "tb_winding_refusal": (C.c_int, [C.c_uint32, C.c_uint64, vp, vp, P(abi.tb_probe_grid), C.c_float, C.c_char_p, C.c_uint32]),
        "tb_host_scene_winding": (C.c_int, [vp, C.c_uint32, C.c_uint64, vp, C.c_float, vp]),
        "tb_update_positions": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
        "tb_update_normals": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
        "tb_set_instance_transforms": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "tb_commit_geometry": (C.c_int, [vp, C.c_uint32]),
        "tb_geometry_vertex_range": (C.c_int, [vp, C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
        "tb_load_meshes": (C.c_int, [vp, P(abi.tb_scene_desc)]),
        "tb_meshes_refusal": (C.c_int, [P(abi.tb_scene_desc), C.c_char_p, C.c_uint32]),
        "tb_host_scene_from_meshes": (C.c_int, [P(abi.tb_scene_desc), C.c_int, P(vp), C.c_char_p, C.c_uint32]),
        "tb_host_smooth_normals": (C.c_int, [vp, C.c_uint32, vp, C.c_uint32, vp]),
        "tb_recompute_normals": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "tb_default_compare_settings": (None, [P(abi.tb_compare_settings)]),
        "tb_run_compare": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, P(abi.tb_compare_settings), P(abi.tb_compare_result), vp, vp]),
        "tb_set_reference": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "tb_compare": (C.c_int, [vp, C.c_uint32, P(abi.tb_compare_settings), P(abi.tb_compare_result), vp, vp]),
        "tb_nn_weights_info": (C.c_int, [C.c_char_p, P(abi.tb_nn_info), C.c_char_p, C.c_uint32]),
        "tb_neural_load": (C.c_int, [vp, C.c_char_p]),
        "tb_run_conv3x3": (C.c_int, [vp, P(abi.tb_conv3x3_desc)] + [vp] * 5),
        "tb_run_neural": (C.c_int, [vp, C.c_uint32, C.c_uint32] + [vp] * 4),
        "tb_denoise_neural": (C.c_int, [vp, P(abi.tb_post_settings), vp, vp]),
        "tb_run_nn_pack": (C.c_int, [vp] + [C.c_uint32] * 5 + [vp] * 4),
        "tb_run_nn_unpack": (C.c_int, [vp] + [C.c_uint32] * 4 + [vp, vp]),
        "tb_run_nn_resolve_aux": (C.c_int, [vp, C.c_uint32, C.c_uint32] + [vp] * 4),
        "tb_run_nn_to_rgba8": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp]),
        "tb_sr_weights_info": (C.c_int, [C.c_char_p, P(abi.tb_sr_info), C.c_char_p, C.c_uint32]),
        "tb_sr_read_layer": (C.c_int, [C.c_char_p, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32]),
        "tb_sr_load": (C.c_int, [vp, C.c_char_p]),
        "tb_run_conv": (C.c_int, [vp, P(abi.tb_conv_desc)] + [vp] * 5),
        "tb_run_sr_finish": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, vp]),
        "tb_run_sr": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp]),
        "tb_upscale_neural": (C.c_int, [vp, P(abi.tb_post_settings), vp, vp]),
        "tb_variant_stash_entries": (C.c_int, [C.c_char_p]),
        "tb_frame_groups": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32)]),
        "tb_state_begin": (C.c_int, [vp, C.c_uint32, C.c_uint32, P(abi.tb_output_settings), C.c_float, C.c_uint32]),
        "tb_state_save": (C.c_int, [vp, C.c_char_p]),
        "tb_state_load": (C.c_int, [vp, C.c_char_p, C.c_uint32]),
        "tb_accum_digest": (C.c_int, [vp, P(C.c_uint64)]),
        "tb_scene_digest": (C.c_int, [vp, P(C.c_uint64)]),
        "tb_state_info_read": (C.c_int, [C.c_char_p, P(abi.tb_state_info), C.c_char_p, C.c_uint32]),
        "tb_state_read_host": (C.c_int, [C.c_char_p, P(abi.tb_state_info), vp, vp, C.c_char_p, C.c_uint32]),
        "tb_state_write_host": (C.c_int, [C.c_char_p, P(abi.tb_state_info), vp, vp]),
        "tb_state_digest_host": (C.c_uint64, [vp, C.c_uint64]),
        "tb_host_scene_digest": (C.c_int, [vp, P(C.c_uint64)]),
        "tb_host_scene_load": (C.c_int, [C.c_char_p, C.c_int, C.c_int, P(vp), C.c_char_p, C.c_uint32]),
        "tb_host_scene_procedural": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, P(vp), C.c_char_p, C.c_uint32]),
        "tb_host_scene_free": (None, [vp]),
        "tb_host_pbrt_dump": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32]),
        "tb_host_scene_view_get": (C.c_int, [vp, P(abi.TbSceneView)]),
        "tb_host_scene_camera": (C.c_int, [vp, P(abi.tb_camera)]),
        "tb_host_scene_info": (C.c_int, [vp, P(abi.tb_scene_info)]),
        "tb_host_scene_frame_constants": (C.c_int, [vp, P(abi.tb_output_settings), C.c_uint32, C.c_float, P(abi.TbPerFrameConstants)]),
        "tb_host_scene_layout_b": (C.c_int, [vp, P(P(abi.TbNodeB)), P(C.c_uint32), P(P(abi.TbTriB)), P(C.c_uint32), P(C.c_uint32)]),
        "tb_host_scene_lds_image": (C.c_int, [vp, P(C.c_uint8), C.c_uint32, P(abi.tb_lds_image_info)]),
        "tb_host_scene_tables_in_range": (C.c_int, [P(abi.TbTriB), C.c_uint32, P(C.c_uint32), C.c_uint32, P(C.c_uint32)] + [C.c_uint32] * 3),
        "tb_host_scene_triangles": (C.c_int, [vp, P(P(C.c_float)), P(C.c_uint32), P(P(C.c_uint32)), P(P(C.c_uint32)), P(P(C.c_uint32)), P(P(C.c_uint32)), P(C.c_uint32)]),
        "tb_wave_replay": (C.c_int, [P(C.c_char_p), C.c_uint32, C.c_uint32, P(abi.tb_wave_trips)]),
        "tb_host_scene_wave_walk": (C.c_int, [vp, C.c_uint32, P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_uint32), P(C.c_uint32), C.c_char_p, C.c_uint64]),
        "tb_host_scene_wave_rays": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, P(C.c_float), P(C.c_float), P(C.c_float), C.c_uint32]),
        "tb_host_scene_wave_cost": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, P(abi.tb_wave_trips)]),
        "tb_host_scene_wave_stage": (C.c_int, [vp, P(abi.tb_wave_stage_info)]),
        "tb_host_scene_wave_search": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, P(abi.tb_wave_stage_info)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here == the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    L._tb_exports = sorted(sig)
    _lib = L
    return L


def GetDefaultOutputSettings():
    """TracerBoy::GetDefaultOutputSettings (TracerBoy.h:290-360)."""
    s = abi.tb_output_settings()
    lib().tb_default_output_settings(C.byref(s))
    return s


def GetDefaultDenoiserSettings():
    """GetDefaultOutputSettings().m_denoiserSettings (TracerBoy.h:338-344)."""
    s = abi.tb_denoiser_settings()
    lib().tb_default_denoiser_settings(C.byref(s))
    return s


def GetDefaultPostProcessSettings():
    """GetDefaultOutputSettings().m_postProcessSettings (TracerBoy.h:309-313): exposure 1, AGX punchy, gamma and auto exposure on."""
    s = abi.tb_post_settings()
    lib().tb_default_post_settings(C.byref(s))
    return s


def GetDefaultCompareSettings():
    """The image-quality metrics' defaults (tb_default_compare_settings): peak 1, rel_epsilon 0.01, SSIM on."""
    s = abi.tb_compare_settings()
    lib().tb_default_compare_settings(C.byref(s))
    return s


COMPARE_FIELDS = tuple(n for n, _ in abi.tb_compare_result._fields_)


def FsrConstants(in_width, in_height, out_width, out_height, sharpness=0.2):
    """FsrEasuCon(in, in, out) + FsrRcasCon(sharpness in stops) as the library computes them (tb_fsr_constants; host only, no device)."""
    k = abi.TbFsrConstants()
    rc = lib().tb_fsr_constants(in_width, in_height, out_width, out_height, sharpness, C.byref(k))
    if rc != 0:
        raise TracerBoyError(rc, "tb_fsr_constants: a size is 0 or the sharpness is not finite")
    return k


def GetDefaultVisualizeSettings():
    """GetDefaultOutputSettings().m_debugSettings' ray visualiser part (TracerBoy.h:303-306): RayWidth 0.01, RayDepth 10, RayCount 0 = all."""
    s = abi.tb_visualize_settings()
    lib().tb_default_visualize_settings(C.byref(s))
    return s


def VisualizeConstants(camera, width, height, settings=None):
    """VisualizationRaysConstants as the library fills them for a camera, a picture size and settings (tb_visualize_constants; host only, no device)."""
    k = abi.TbVisualizeConstants()
    rc = lib().tb_visualize_constants(C.byref(camera), width, height, C.byref(settings) if settings is not None else None, C.byref(k))
    if rc != 0:
        raise TracerBoyError(rc, "tb_visualize_constants: a size is 0")
    return k


# the records of the path inspector as numpy sees them (the layouts of TbPathFrame and TbVisualizerRay)
# ray queries (tb_trace_rays; tb_abi.h TbQueryRay / TbQueryHit)
RAYS_CLOSEST, RAYS_OCCLUDED, RAYS_DEVICE = 0, 1, 0x100
QUERY_RAY_DISABLED = 1
QUERY_RAY_DTYPE = np.dtype([("Origin", np.float32, 3), ("TMax", np.float32), ("Direction", np.float32, 3), ("Flags", np.uint32)])
QUERY_HIT_DTYPE = np.dtype([("T", np.float32), ("U", np.float32), ("V", np.float32), ("Prim", np.uint32), ("Geom", np.uint32), ("Material", np.int32),
                            ("UV", np.float32, 2), ("Normal", np.float32, 3), ("Pad", np.uint32)])


def make_query_rays(origins, dirs, tmax=np.inf, disabled=None):
    """(n, 3) origins and directions packed into QUERY_RAY_DTYPE; tmax: a scalar or n values (inf: the renderer's ray); disabled: n booleans."""
    o = np.asarray(origins, np.float32); d = np.asarray(dirs, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("make_query_rays: origins and dirs are (n, 3) arrays of one length")
    rays = np.zeros(o.shape[0], QUERY_RAY_DTYPE)
    rays["Origin"] = o; rays["Direction"] = d
    rays["TMax"] = np.broadcast_to(np.asarray(tmax, np.float32), (o.shape[0],))
    if disabled is not None:
        rays["Flags"] = np.where(np.broadcast_to(np.asarray(disabled, bool), (o.shape[0],)), QUERY_RAY_DISABLED, 0)
    return rays


def _is_torch_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _torch_sync(device):
    """What torch has enqueued on its current stream of the device is done: the library reads and writes a tensor's memory on a stream of its own."""
    import torch
    torch.cuda.current_stream(device).synchronize()


def _is_rows(dims, lead, columns):
    return len(dims) >= 2 and dims[-1] == columns and (len(dims) == 2 if lead is None else tuple(dims[:-1]) == lead)


def _rows_wanted(lead, columns, record_dtype=None):
    """The words of _check_array's refusals: nothing is formatted for an array that passes."""
    n_text = "n" if lead is None else ", ".join(str(r) for r in lead)
    records = "" if record_dtype is None else "%d-B records of shape (%s,) or " % (record_dtype.itemsize, n_text)
    return "%sfloat32 of shape (%s, %d)" % (records, n_text, columns)


def _check_array(what, name, a, device, *, columns, record_dtype=None, align=4, rows=None, written=False, allow_tensor=True):
    """One array of a call, checked before any library call (a wrong array must never reach a kernel as a wrong pointer): True for a torch tensor
    (the device path), False for a numpy array (the host path); ValueError otherwise.  A tensor is float32 of shape (n, columns), contiguous, on
    cuda:`device`, the context's, and `align`-B aligned.  A numpy array is float32 of that shape or, where the call has records, `record_dtype` of
    shape (n,); C-contiguous; writeable where the call writes it.  rows: what stands for n -- a number, or a tuple for an array of more dimensions."""
    lead = None if rows is None else rows if isinstance(rows, tuple) else (rows,)
    if allow_tensor and _is_torch_tensor(a):
        import torch
        if a.dtype != torch.float32 or not _is_rows(tuple(a.shape), lead, columns):
            raise ValueError("%s: the tensor %s is %s, not %s %s" % (what, name, _rows_wanted(lead, columns), a.dtype, tuple(a.shape)))
        if not a.is_contiguous():
            raise ValueError("%s: the tensor %s is not contiguous" % (what, name))
        if a.device.type != "cuda" or a.device.index != device:
            raise ValueError("%s: the tensor %s is on %s, the context on cuda:%d" % (what, name, a.device, device))
        if a.data_ptr() % align:
            raise ValueError("%s: the tensor %s is not %d-B aligned" % (what, name, align))
        return True
    if not isinstance(a, np.ndarray):
        raise ValueError("%s: %s is a numpy array%s, not %s" % (what, name, " or a torch tensor" if allow_tensor else "", type(a).__name__))
    records = record_dtype is not None and a.dtype == record_dtype
    if not (a.ndim == 1 and (lead is None or a.shape == lead) if records else a.dtype == np.float32 and _is_rows(a.shape, lead, columns)):
        raise ValueError("%s: %s is %s, not %s %s" % (what, name, _rows_wanted(lead, columns, record_dtype), a.dtype, a.shape))
    if not a.flags["C_CONTIGUOUS"] or (written and not a.flags["WRITEABLE"]):
        raise ValueError("%s: %s is not contiguous%s" % (what, name, " and writeable" if written else ""))
    return False


def _check_query_rays(rays, mode, device):
    if mode not in (RAYS_CLOSEST, RAYS_OCCLUDED):
        raise ValueError("TraceRays: mode is RAYS_CLOSEST or RAYS_OCCLUDED, not %r" % (mode,))
    return _check_array("TraceRays", "rays", rays, device, columns=8, record_dtype=QUERY_RAY_DTYPE, align=16)


# radiance queries (tb_trace_radiance / tb_make_camera_rays; tb_abi.h TbRadianceRay / TbRadianceCall)
RADIANCE_RAY, RADIANCE_HEMISPHERE, RADIANCE_DEVICE, RADIANCE_ACCUMULATE = 0, 1, 0x100, 0x200
RADIANCE_RAY_DTYPE = np.dtype([("Origin", np.float32, 3), ("SeedX", np.float32), ("Direction", np.float32, 3), ("SeedY", np.float32)])
assert RADIANCE_RAY_DTYPE.itemsize == 32


def make_radiance_rays(origins, dirs_or_normals, seed_xy=None):
    """(n, 3) origins and unit directions (hemisphere mode: unit normals) packed into RADIANCE_RAY_DTYPE; seed_xy: (n, 2) numbers that stand where the
    pixel coordinates stand in the renderer's seed -- by default (i % 4096, i // 4096), distinct whole numbers per ray."""
    o = np.asarray(origins, np.float32); d = np.asarray(dirs_or_normals, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("make_radiance_rays: origins and directions are (n, 3) arrays of one length")
    n = o.shape[0]
    if seed_xy is None:
        i = np.arange(n, dtype=np.int64)
        seed = np.stack([i % 4096, i // 4096], axis=1).astype(np.float32)
    else:
        seed = np.asarray(seed_xy, np.float32)
        if seed.shape != (n, 2):
            raise ValueError("make_radiance_rays: seed_xy is an (n, 2) array")
    rays = np.zeros(n, RADIANCE_RAY_DTYPE)
    rays["Origin"] = o; rays["Direction"] = d; rays["SeedX"] = seed[:, 0]; rays["SeedY"] = seed[:, 1]
    return rays


def _check_count(what, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > hi:
        raise ValueError("%s: %s is a whole number in [%d, %d], not %r" % (what, name, lo, hi, v))
    return int(v)


def _check_radiance_call(rays, samples, first_sample, seed_advance, mode, out, device):
    """What TraceRadiance accepts, checked before any library call: True for torch tensors (the device path), False for numpy arrays (the host
    path); ValueError otherwise."""
    if isinstance(mode, bool) or mode not in (RADIANCE_RAY, RADIANCE_HEMISPHERE):
        raise ValueError("TraceRadiance: mode is RADIANCE_RAY or RADIANCE_HEMISPHERE, not %r" % (mode,))
    _check_count("TraceRadiance", "samples", samples, 1, 1 << 24)
    _check_count("TraceRadiance", "first_sample", first_sample, 0, (1 << 32) - samples)
    if isinstance(seed_advance, bool) or not isinstance(seed_advance, (int, float, np.integer, np.floating)) or not np.isfinite(seed_advance):
        raise ValueError("TraceRadiance: seed_advance is a finite number, not %r" % (seed_advance,))
    on_device = _check_array("TraceRadiance", "rays", rays, device, columns=8, record_dtype=RADIANCE_RAY_DTYPE, align=16)
    if out is not None and _check_array("TraceRadiance", "out", out, device, columns=4, align=16, rows=int(rays.shape[0]), written=True) != on_device:
        raise ValueError("TraceRadiance: rays and out are both numpy arrays or both torch tensors")
    return on_device


def _refusal(name, *args, room=96):
    """A pure tb_*_refusal of the library asked: None, or the reason it wrote into the `room` bytes behind its arguments."""
    why = C.create_string_buffer(room)
    return None if getattr(lib(), name)(*args, why, room) == 0 else why.value.decode()


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def _address(a):
    return C.c_void_p(a or None)


def RadianceRefusal(call, n, rays_address, out_address):
    """tb_radiance_refusal (host only): why tb_trace_radiance refuses these arguments before it looks at its context -- None, or the reason."""
    return _refusal("tb_radiance_refusal", _ref(call), n, _address(rays_address), _address(out_address))


# lightmap baking (tb_bake_lightmap .. tb_run_bake_dilate; tb_abi.h TbBakeTexel)
BAKE_DEVICE, BAKE_ACCUMULATE = 0x100, 0x200
BAKE_MAX_SIDE, BAKE_MAX_DILATE, BAKE_NO_TRIANGLE = 8192, 16, 0xffffffff
BAKE_TEXEL_DTYPE = np.dtype([("triangle", np.uint32), ("cls", np.uint32), ("w0", np.float32), ("w1", np.float32)])
assert BAKE_TEXEL_DTYPE.itemsize == 16


def _check_bake_call(width, height, samples, uv, first_sample, dilate, accumulate, out, device):
    """What BakeLightmap accepts, checked before any library call: True for the device path (uv and / or out are torch tensors), False for the host
    path (numpy arrays or None); ValueError otherwise.  That uv has one pair per vertex of the scene is checked by the caller."""
    _check_count("BakeLightmap", "width", width, 1, BAKE_MAX_SIDE)
    _check_count("BakeLightmap", "height", height, 1, BAKE_MAX_SIDE)
    _check_count("BakeLightmap", "samples", samples, 1, 1 << 24)
    _check_count("BakeLightmap", "first_sample", first_sample, 0, (1 << 32) - samples)
    _check_count("BakeLightmap", "dilate", dilate, 0, BAKE_MAX_DILATE)
    if not isinstance(accumulate, (bool, np.bool_)):
        raise ValueError("BakeLightmap: accumulate is True or False, not %r" % (accumulate,))
    kinds = set()
    if uv is not None:
        kinds.add(_check_array("BakeLightmap", "uv", uv, device, columns=2))
    if out is not None:
        kinds.add(_check_array("BakeLightmap", "out", out, device, columns=4, align=16, rows=(height, width), written=True))
    if len(kinds) > 1:
        raise ValueError("BakeLightmap: uv and out are both numpy arrays or both torch tensors")
    return kinds == {True}


def BakeRefusal(call, uv_address, out_address):
    """tb_bake_refusal (host only): why tb_bake_lightmap refuses these arguments before it looks at its context -- None, or the reason."""
    return _refusal("tb_bake_refusal", _ref(call), _address(uv_address), _address(out_address))


# light probes (tb_bake_probes .. tb_run_probe_project; tb_abi.h TbProbe, tb_probe_grid)
PROBES_DEVICE, PROBES_ACCUMULATE, PROBES_KEEP_MAPS = 0x100, 0x200, 0x400
PROBE_MIN_RES, PROBE_MAX_RES, PROBE_MAX_PROBES = 2, 64, 1 << 24
PROBE_DTYPE = np.dtype([("SH", np.float32, (9, 3)), ("Weight", np.float32), ("Hits", np.float32), ("Backfaces", np.float32), ("MinDistance", np.float32),
                        ("MeanDistance", np.float32)])
assert PROBE_DTYPE.itemsize == 128


class ProbeGrid:
    """A grid of probes: count = (nx, ny, nz) probes, probe (i, j, k) with the number (k * ny + j) * nx + i at origin + (i, j, k) * spacing."""

    def __init__(self, origin, spacing, count):
        o = np.asarray(origin, np.float64); sp = np.asarray(spacing, np.float64)
        if o.shape != (3,) or sp.shape != (3,) or not np.isfinite(o).all() or not np.isfinite(sp).all():
            raise ValueError("ProbeGrid: origin and spacing are three finite numbers each")
        if len(count) != 3:
            raise ValueError("ProbeGrid: count is three whole numbers")
        self.count = tuple(_check_count("ProbeGrid", "count", v, 1, PROBE_MAX_PROBES) for v in count)
        if self.count[0] * self.count[1] * self.count[2] > PROBE_MAX_PROBES:
            raise ValueError("ProbeGrid: more than 2^24 probes")
        self.origin = tuple(float(np.float32(v)) for v in o); self.spacing = tuple(float(np.float32(v)) for v in sp)

    @classmethod
    def in_bounds(cls, lo, hi, count):
        """The grid whose probes sit at the centres of count[0] x count[1] x count[2] equal cells of the box [lo, hi]."""
        lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64); k = np.asarray(count, np.float64)
        if lo.shape != (3,) or hi.shape != (3,) or k.shape != (3,) or (k < 1).any():
            raise ValueError("ProbeGrid.in_bounds: lo, hi and count have three entries each")
        cell = (hi - lo) / k
        return cls(lo + 0.5 * cell, cell, count)

    @property
    def n(self):
        return self.count[0] * self.count[1] * self.count[2]

    def c_struct(self):
        return abi.tb_probe_grid((C.c_float * 3)(*self.origin), (C.c_float * 3)(*self.spacing), (C.c_uint32 * 3)(*self.count))


def probe_grid_positions(grid):
    """The (n, 3) float32 positions of a ProbeGrid's probes in its numbering: origin + (i, j, k) * spacing, one rounded product and one rounded sum."""
    nx, ny, nz = grid.count
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.asarray(grid.origin, np.float32) + ijk * np.asarray(grid.spacing, np.float32))


def _check_probe_call(positions, resolution, samples, first_sample, first_number, keep_maps, accumulate, device):
    """What BakeProbes accepts, checked before any library call: True for a torch tensor of positions (the device path), False for a numpy array."""
    _check_count("BakeProbes", "resolution", resolution, PROBE_MIN_RES, PROBE_MAX_RES)
    _check_count("BakeProbes", "samples", samples, 1, 1 << 24)
    _check_count("BakeProbes", "first_sample", first_sample, 0, (1 << 32) - samples)
    for name, v in (("keep_maps", keep_maps), ("accumulate", accumulate)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("BakeProbes: %s is True or False, not %r" % (name, v))
    on_device = _check_array("BakeProbes", "positions", positions, device, columns=3)
    n = int(positions.shape[0])
    if n > PROBE_MAX_PROBES or n * resolution * resolution > 1 << 31:
        raise ValueError("BakeProbes: %d probes of %d x %d rays are more than 2^24 probes or 2^31 rays" % (n, resolution, resolution))
    _check_count("BakeProbes", "first_number", first_number, 0, PROBE_MAX_PROBES - n)
    return on_device


def ProbesRefusal(call, positions_address, probes_address):
    """tb_probes_refusal (host only): why tb_bake_probes refuses these arguments before it looks at its context -- None, or the reason."""
    return _refusal("tb_probes_refusal", _ref(call), _address(positions_address), _address(probes_address))


def sh9_irradiance(probe, normal):
    """tb_sh9_irradiance (host only): the float32 (3,) irradiance of one PROBE_DTYPE record at a unit normal, by the sampler's own arithmetic."""
    rec = np.ascontiguousarray(probe, PROBE_DTYPE).reshape(1)
    nrm = np.ascontiguousarray(normal, np.float32)
    if nrm.shape != (3,):
        raise ValueError("sh9_irradiance: the normal has three components")
    out = np.empty(3, np.float32)
    if lib().tb_sh9_irradiance(_np_ptr(rec), _np_ptr(nrm), _np_ptr(out)) != 0:
        raise ValueError("sh9_irradiance: refused")
    return out


def probe_directions(resolution):
    """tb_probe_directions (host only): the float32 (M * M, 3) unit directions and (M * M,) solid angles of an M x M octahedral map."""
    _check_count("probe_directions", "resolution", resolution, PROBE_MIN_RES, PROBE_MAX_RES)
    d = np.empty((resolution * resolution, 3), np.float32); w = np.empty(resolution * resolution, np.float32)
    if lib().tb_probe_directions(resolution, _np_ptr(d), _np_ptr(w)) != 0:
        raise ValueError("probe_directions: refused")
    return d, w


# point queries (tb_nearest_points, tb_bake_distance_field; tb_abi.h TbQueryPoint / TbNearest; the rule: include/tb_nearest.h)
NEAREST_SIGNED, NEAREST_DEVICE, NEAREST_HOST_BRUTE, NEAREST_HOST_WALK = 1, 0x100, 0x1000, 0x2000
NEAREST_NONE = 0xffffffff
QUERY_POINT_DTYPE = np.dtype([("Position", np.float32, 3), ("MaxDistance", np.float32)])
NEAREST_DTYPE = np.dtype([("Point", np.float32, 3), ("Distance", np.float32), ("U", np.float32), ("V", np.float32), ("Prim", np.uint32), ("Geom", np.uint32)])
assert QUERY_POINT_DTYPE.itemsize == 16 and NEAREST_DTYPE.itemsize == 32


def make_query_points(positions, max_distance=np.inf):
    """(n, 3) positions packed into QUERY_POINT_DTYPE; max_distance: a scalar or n values (inf: every triangle counts)."""
    p = np.asarray(positions, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("make_query_points: positions are an (n, 3) array")
    points = np.zeros(p.shape[0], QUERY_POINT_DTYPE)
    points["Position"] = p
    points["MaxDistance"] = np.broadcast_to(np.asarray(max_distance, np.float32), (p.shape[0],))
    return points


def _check_flag(what, name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s: %s is True or False, not %r" % (what, name, v))
    return bool(v)


def _check_query_points(what, points, device, allow_tensor=True):
    return _check_array(what, "points", points, device, columns=4, record_dtype=QUERY_POINT_DTYPE, align=16, allow_tensor=allow_tensor)


def _check_distance_field(grid, signed, max_distance, device):
    if not isinstance(grid, ProbeGrid):
        raise ValueError("BakeDistanceField: grid is a ProbeGrid, not %s" % type(grid).__name__)
    _check_flag("BakeDistanceField", "signed", signed); _check_flag("BakeDistanceField", "device", device)
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)):
        raise ValueError("BakeDistanceField: max_distance is a number, not %r" % (max_distance,))
    if grid.n > 1 << 31:
        raise ValueError("BakeDistanceField: more than 2^31 cells")


def NearestRefusal(flags, n, points_address, out_address, grid=None):
    """tb_nearest_refusal (host only): why tb_nearest_points -- with a grid (abi.tb_probe_grid): tb_bake_distance_field -- refuses these arguments before
    it looks at its context: None, or the reason."""
    return _refusal("tb_nearest_refusal", flags, n, _address(points_address), _address(out_address), _ref(grid))


# winding numbers (tb_winding_numbers .. tb_bake_distance_field_winding; the rule: include/tb_winding.h)
WINDING_DEVICE, WINDING_HOST_BRUTE, WINDING_HOST_WALK = 0x100, 0x1000, 0x2000
WINDING_BETA = 3.0   # the smallest of 2, 3, 4 whose measured error bound is below 0.25 (tests/winding_cases.py W_BETA_TOL)


def winding_inside(w):
    """tb_winding_inside of include/tb_winding.h: |w| >= 0.5, whichever way the mesh faces; a NaN is not inside."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(w, np.float32)) >= np.float32(0.5)


def _check_beta(what, beta, name="beta"):
    """beta is a number >= 1 (inf: the exact form); ValueError otherwise"""
    if isinstance(beta, (bool, np.bool_)) or not isinstance(beta, (int, float, np.integer, np.floating)) or not float(beta) >= 1.0:
        raise ValueError("%s: %s is a number >= 1, not %r" % (what, name, beta))
    return float(beta)


def WindingRefusal(flags, n, points_address, out_address, grid=None, beta=WINDING_BETA):
    """tb_winding_refusal (host only): why tb_winding_numbers -- with a grid (abi.tb_probe_grid): tb_bake_winding_field -- refuses these arguments
    before it looks at its context: None, or the reason."""
    return _refusal("tb_winding_refusal", flags, n, _address(points_address), _address(out_address), _ref(grid), beta)


# dynamic scenes (tb_update_positions .. tb_commit_geometry)
UPDATE_DEVICE, GEOMETRY_REBUILD = 0x100, 1


def _check_vertex_array(what, a, first, device):
    """What UpdatePositions / UpdateNormals accept, checked before any library call: True for a torch tensor (the device path), False for a numpy
    array (the host path); ValueError otherwise."""
    if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or first < 0 or first > 0xffffffff:
        raise ValueError("%s: first is a vertex number, not %r" % (what, first))
    if _is_torch_tensor(a):
        import torch
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError("%s: a tensor is float32 of shape (n, 3), not %s %s" % (what, a.dtype, tuple(a.shape)))
        if not a.is_contiguous():
            raise ValueError("%s: the tensor is not contiguous" % what)
        if a.device.type != "cuda" or a.device.index != device:
            raise ValueError("%s: the tensor is on %s, the context on cuda:%d" % (what, a.device, device))
    elif not isinstance(a, np.ndarray):
        raise ValueError("%s: a numpy array or a torch tensor, not %s" % (what, type(a).__name__))
    elif a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: an array is float32 of shape (n, 3), not %s %s" % (what, a.dtype, a.shape))
    elif not a.flags["C_CONTIGUOUS"]:
        raise ValueError("%s: the array is not contiguous" % what)
    if first + int(a.shape[0]) > 0xffffffff:
        raise ValueError("%s: first + n is no vertex number" % what)
    return _is_torch_tensor(a)


# scenes from arrays (tb_load_meshes)
MESH_NORMALS_FLAT, MESH_NORMALS_SMOOTH, MESH_DEVICE = 0, 1, 0x100


class Mesh:
    """One mesh of a scene from arrays.  positions (n, 3) float32, indices (m, 3) uint32, normals (n, 3) / uvs (n, 2) float32 or None: numpy arrays,
    or all of them contiguous torch tensors on the context's device (indices then uint32 or non-negative int32).  material: an index into the call's
    material table.  smooth: read without normals -- True: include/tb_normals.h's smooth normals, False: the loader's flat ones."""

    def __init__(self, positions, indices, normals=None, uvs=None, material=0, smooth=False):
        self.positions, self.indices, self.normals, self.uvs, self.material, self.smooth = positions, indices, normals, uvs, material, smooth


def _check_meshes(what, meshes, device):
    """What LoadMeshes / HostScene.from_meshes accept, checked before any library call: True when the arrays are torch tensors (the device path), False for
    numpy arrays; ValueError otherwise (device None: host arrays only)."""
    meshes = list(meshes)
    kinds = set()
    for k, m in enumerate(meshes):
        if not isinstance(m, Mesh):
            raise ValueError("%s: mesh %d is an api.Mesh, not %s" % (what, k, type(m).__name__))
        if isinstance(m.material, bool) or not isinstance(m.material, (int, np.integer)) or m.material < 0 or m.material > 0xffffffff:
            raise ValueError("%s: mesh %d: material is an index, not %r" % (what, k, m.material))
        for name, a, cols, optional in (("positions", m.positions, 3, False), ("indices", m.indices, 3, False), ("normals", m.normals, 3, True), ("uvs", m.uvs, 2, True)):
            if a is None:
                if optional:
                    continue
                raise ValueError("%s: mesh %d: %s is missing" % (what, k, name))
            index = name == "indices"
            if _is_torch_tensor(a):
                import torch
                kinds.add("torch")
                if device is None:
                    raise ValueError("%s: mesh %d: %s is a torch tensor; a host scene takes numpy arrays" % (what, k, name))
                ok = (a.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))) if index else a.dtype == torch.float32
                if not ok or a.dim() != 2 or a.shape[1] != cols:
                    raise ValueError("%s: mesh %d: %s is %s of shape (n, %d), not %s %s" % (what, k, name, "uint32 / int32" if index else "float32", cols, a.dtype, tuple(a.shape)))
                if not a.is_contiguous():
                    raise ValueError("%s: mesh %d: the tensor %s is not contiguous" % (what, k, name))
                if a.device.type != "cuda" or a.device.index != device:
                    raise ValueError("%s: mesh %d: %s is on %s, the context on cuda:%d" % (what, k, name, a.device, device))
            elif isinstance(a, np.ndarray):
                kinds.add("numpy")
                if a.dtype != (np.uint32 if index else np.float32) or a.ndim != 2 or a.shape[1] != cols:
                    raise ValueError("%s: mesh %d: %s is %s of shape (n, %d), not %s %s" % (what, k, name, "uint32" if index else "float32", cols, a.dtype, a.shape))
                if not a.flags["C_CONTIGUOUS"]:
                    raise ValueError("%s: mesh %d: the array %s is not contiguous" % (what, k, name))
            else:
                raise ValueError("%s: mesh %d: %s is a numpy array or a torch tensor, not %s" % (what, k, name, type(a).__name__))
            if not index and name != "positions" and int(a.shape[0]) != int(m.positions.shape[0]):
                raise ValueError("%s: mesh %d: %s has %d rows, the mesh %d vertices" % (what, k, name, a.shape[0], m.positions.shape[0]))
            if int(a.shape[0]) > 0xffffffff:
                raise ValueError("%s: mesh %d: %s has too many rows" % (what, k, name))
    if len(kinds) > 1:
        raise ValueError("%s: numpy arrays and torch tensors are mixed" % what)
    on_device = kinds == {"torch"}
    if on_device:
        import torch
        for k, m in enumerate(meshes):
            if m.indices.dtype == torch.int32 and m.indices.numel() and int(m.indices.min()) < 0:
                raise ValueError("%s: mesh %d: an int32 index is negative" % (what, k))
    return on_device


def _scene_desc(what, meshes, materials, camera, environment, env_scale, film, device):
    """(tb_scene_desc, what keeps its arrays alive) from the Python arguments; every check of _check_meshes first."""
    meshes = list(meshes)
    on_device = _check_meshes(what, meshes, device)
    keep = []
    mats = list(materials)
    for i, mt in enumerate(mats):
        if not isinstance(mt, abi.TbMaterial):
            raise ValueError("%s: material %d is a TbMaterial, not %s" % (what, i, type(mt).__name__))
    if environment is not None:
        if not isinstance(environment, np.ndarray) or environment.dtype != np.float32 or environment.ndim != 3 or environment.shape[2] != 4 or \
                not environment.flags["C_CONTIGUOUS"]:
            raise ValueError("%s: environment is a contiguous float32 numpy array of shape (H, W, 4)" % what)
    if len(tuple(env_scale)) != 3 or len(tuple(film)) != 2:
        raise ValueError("%s: env_scale has 3 values and film 2" % what)
    ptr = (lambda a: C.c_void_p(a.data_ptr() or None)) if on_device else _np_ptr
    md = (abi.tb_mesh_desc * max(len(meshes), 1))()
    for k, m in enumerate(meshes):
        md[k].positions = ptr(m.positions); md[k].n_vertices = int(m.positions.shape[0])
        md[k].indices = ptr(m.indices); md[k].n_triangles = int(m.indices.shape[0])
        md[k].normals_or_null = ptr(m.normals) if m.normals is not None else None
        md[k].uvs_or_null = ptr(m.uvs) if m.uvs is not None else None
        md[k].material = int(m.material); md[k].normals_mode = MESH_NORMALS_SMOOTH if m.smooth else MESH_NORMALS_FLAT
        keep.append((m.positions, m.indices, m.normals, m.uvs))
    ma = (abi.TbMaterial * max(len(mats), 1))(*mats)
    d = abi.tb_scene_desc()
    d.meshes = C.cast(md, C.POINTER(abi.tb_mesh_desc)) if meshes else None; d.n_meshes = len(meshes)
    d.materials = C.cast(ma, C.POINTER(abi.TbMaterial)) if mats else None; d.n_materials = len(mats)
    if camera is not None:
        cam = abi.tb_camera.from_buffer_copy(camera); keep.append(cam)
        d.camera_or_null = C.pointer(cam)
    if environment is not None:
        d.env_rgba_or_null = _np_ptr(environment); d.env_height, d.env_width = int(environment.shape[0]), int(environment.shape[1])
        keep.append(environment)
    d.env_scale = (C.c_float * 3)(*[float(x) for x in env_scale])
    d.film_width, d.film_height = int(film[0]), int(film[1])
    d.flags = MESH_DEVICE if on_device else 0
    keep += [md, ma]
    return d, keep, on_device


def MeshesRefusal(desc):
    """tb_meshes_refusal (host only, pure): why tb_load_meshes refuses this tb_scene_desc before it looks at its context -- None, or the reason."""
    return _refusal("tb_meshes_refusal", _ref(desc), room=160)


def HostSmoothNormals(positions, indices, out=None):
    """tb_host_smooth_normals: include/tb_normals.h's rule over one mesh -- (n, 3) float32 positions, (m, 3) uint32 indices -> (n, 3) normals; a
    vertex that no triangle names keeps what `out` holds ((0, 1, 0) when out is None)."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); i = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    if out is None:
        out = np.zeros_like(p); out[:, 1] = 1.0
    rc = lib().tb_host_smooth_normals(_np_ptr(p), p.shape[0], _np_ptr(i), i.shape[0], _np_ptr(out))
    if rc != 0:
        raise TracerBoyError(rc, "tb_host_smooth_normals: a null pointer or an index at or past the vertices")
    return out


PATH_FRAME_DTYPE = np.dtype([("sum", np.float32, 4), ("frame", np.uint32), ("first_ray", np.uint32), ("num_rays", np.uint32), ("flags", np.uint32)])
VISUALIZER_RAY_DTYPE = np.dtype([("Origin", np.float32, 3), ("Direction", np.float32, 3), ("HitT", np.float32), ("BounceCount", np.float32)])
assert PATH_FRAME_DTYPE.itemsize == 32 and VISUALIZER_RAY_DTYPE.itemsize == 32


NEURAL_LAYERS = ("enc_conv0", "enc_conv1", "enc_conv2", "enc_conv3", "enc_conv4", "enc_conv5a", "enc_conv5b", "dec_conv4a", "dec_conv4b", "dec_conv3a",
                 "dec_conv3b", "dec_conv2a", "dec_conv2b", "dec_conv1a", "dec_conv1b", "dec_conv0")


def NeuralWeightsInfo(path):
    """The channel counts of a TZA weights file of the neural still denoiser (tb_nn_weights_info; host only, no device): a tb_nn_info whose
    out_channels / in_channels_of follow NEURAL_LAYERS.  Raises TracerBoyError with code -3 (unreadable) or -4 (the message names the tensor and
    the cause)."""
    info, err = abi.tb_nn_info(), C.create_string_buffer(512)
    rc = lib().tb_nn_weights_info(os.fsencode(path), C.byref(info), err, 512)
    if rc != 0:
        raise TracerBoyError(rc, err.value.decode(errors="replace"))
    return info


SR_LAYERS = ("conv1", "conv2", "conv3", "conv_up1/conv", "conv4", "conv5", "conv6")


def SrWeightsInfo(path):
    """The channel counts and filter sizes of a weights file of the neural 2 x super-resolution (tb_sr_weights_info; host only, no device): a
    tb_sr_info whose arrays follow SR_LAYERS.  Raises TracerBoyError with code -3 (unreadable) or -4 (the message names the tensor and the cause)."""
    info, err = abi.tb_sr_info(), C.create_string_buffer(512)
    rc = lib().tb_sr_weights_info(os.fsencode(path), C.byref(info), err, 512)
    if rc != 0:
        raise TracerBoyError(rc, err.value.decode(errors="replace"))
    return info


def SrReadLayer(path, layer):
    """One layer of such a file as the network uses it (tb_sr_read_layer; host only): (weight (out, in, K, K) float16 with the batch-norm scale
    folded in, bias (out,) float16 or None for the last layer), converted as the reference converts them."""
    info = SrWeightsInfo(path)
    o, i, k = info.out_channels[layer], info.in_channels[layer], info.kernel[layer]
    weight, bias, err = np.empty((o, i, k, k), np.float16), np.empty((o,), np.float16), C.create_string_buffer(512)
    rc = lib().tb_sr_read_layer(os.fsencode(path), layer, _np_ptr(weight), _np_ptr(bias), err, 512)
    if rc != 0:
        raise TracerBoyError(rc, err.value.decode(errors="replace"))
    return weight, (bias if layer < 6 else None)


def VariantWavesHi(name):
    """Waves per SIMD the higher-occupancy copy of feature set `name` is compiled for (0: no such copy; tb_variant_waves_hi)."""
    return int(lib().tb_variant_waves_hi(name.encode()))


def VariantWavesLds(name):
    """Waves per SIMD the copy of feature set `name` for scenes in LDS is compiled for (0: no such copy; tb_variant_waves_lds)."""
    return int(lib().tb_variant_waves_lds(name.encode()))


def VariantStashEntries(name):
    """LDS entries per lane the higher-occupancy copy's frame-group kernels keep behind the stacks (tb_variant_stash_entries)."""
    return int(lib().tb_variant_stash_entries(name.encode()))


def PlanLaunch(**kw):
    """The launch policy of tb_render as a pure function (include/tracerboy_hip.h tb_plan_launch; no device): keyword arguments are
    fields of tb_plan_input over the option defaults; returns the tb_launch_plan."""
    pin = abi.tb_plan_input(); lib().tb_plan_defaults(C.byref(pin))
    for k, v in kw.items():
        if not hasattr(pin, k): raise KeyError(k)
        setattr(pin, k, v)
    plan = abi.tb_launch_plan()
    rc = lib().tb_plan_launch(C.byref(pin), C.byref(plan))
    if rc != 0: raise TracerBoyError(rc, "tb_plan_launch")
    return plan


def WriteImage(path, image):
    """uint8 HxWx4 -> .png, float32 HxWx4 -> .pfm / .exr (tb_write_image_*)."""
    a = np.ascontiguousarray(image)
    h, w = a.shape[:2]
    if a.dtype == np.uint8:
        rc = lib().tb_write_image_rgba8(os.fsencode(path), w, h, _np_ptr(a))
    else:
        a = np.ascontiguousarray(a, np.float32)
        rc = lib().tb_write_image_f32(os.fsencode(path), w, h, _np_ptr(a))
    if rc != 0:
        raise TracerBoyError(rc, "could not write %s" % path)


def DecodeImage(path):
    """The scene loader's texture decoder on its own: (float32 HxWx4, normalized, has_alpha) for .hdr/.pfm/.png/.tga."""
    w, h, n, a = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
    rc = lib().tb_decode_image(os.fsencode(path), C.byref(w), C.byref(h), C.byref(n), C.byref(a), None)
    if rc != 0:
        raise TracerBoyError(rc, (lib().tb_last_error(None) or b"").decode())
    img = np.empty((h.value, w.value, 4), np.float32)
    rc = lib().tb_decode_image(os.fsencode(path), C.byref(w), C.byref(h), C.byref(n), C.byref(a), _np_ptr(img))
    if rc != 0:
        raise TracerBoyError(rc, (lib().tb_last_error(None) or b"").decode())
    return img, bool(n.value), bool(a.value)


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _tensor_ptr(a):
    return C.c_void_p(a.data_ptr() or None)


# -- render-state files, host only: no device, no context ----------------
TB_STATE_REPLACE, TB_STATE_ADD, TB_STATE_ANY_SCENE = 0, 1, 16
STATE_HEADER_BYTES = 256


def StateDigest(words):
    """The digest of include/tb_state.h over the array's bytes as 32-bit words (tb_state_digest_host)."""
    a = np.ascontiguousarray(words)
    assert a.nbytes % 4 == 0, "the digest is defined over 32-bit words"
    return int(lib().tb_state_digest_host(_np_ptr(a), a.nbytes // 4))


def StateInfo(path):
    """The header of a state file (tb_state_info), validated together with the file's length; reads no surface."""
    info, err = abi.tb_state_info(), C.create_string_buffer(512)
    rc = lib().tb_state_info_read(os.fsencode(path), C.byref(info), err, 512)
    if rc != 0:
        raise TracerBoyError(rc, err.value.decode(errors="replace"))
    return info


def ReadStateFile(path):
    """(tb_state_info, output, jittered): the header and the two (H, W, 4) float32 surfaces, checked against the stored digests."""
    info = StateInfo(path)
    out = np.empty((info.height, info.width, 4), np.float32); jit = np.empty_like(out)
    err = C.create_string_buffer(512)
    rc = lib().tb_state_read_host(os.fsencode(path), C.byref(info), _np_ptr(out), _np_ptr(jit), err, 512)
    if rc != 0:
        raise TracerBoyError(rc, err.value.decode(errors="replace"))
    return info, out, jit


def WriteStateFile(path, info, output, jittered):
    """Write a state file from host arrays (tb_state_write_host): width, height and the two digests are taken from the arrays."""
    out = np.ascontiguousarray(output, np.float32); jit = np.ascontiguousarray(jittered, np.float32)
    assert out.ndim == 3 and out.shape[2] == 4 and jit.shape == out.shape
    h = abi.tb_state_info.from_buffer_copy(info)
    h.height, h.width = out.shape[:2]
    rc = lib().tb_state_write_host(os.fsencode(path), C.byref(h), _np_ptr(out), _np_ptr(jit))
    if rc != 0:
        raise TracerBoyError(rc, "could not write state file %s" % path)


class HostScene:
    """Host-only LoadScene (parse + convert + BVH build): no GPU needed, renders nothing."""

    def __init__(self, path=None, procedural=None, bvh_builder=0, flatten_instances=True, flip_texture_uvs=True, reinsertion_passes=None,
                 reinsertion_share=None, presplit=None, wave_tree=None):
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        # the builder word of include/tracerboy_hip.h: builder | (wave_tree + 1) << 6 | (passes + 1) << 8 | share << 16
        if wave_tree is not None:
            bvh_builder |= (1 + (1 if wave_tree else 0)) << 6
        if reinsertion_passes is not None:
            bvh_builder |= (int(reinsertion_passes) + 1) << 8
        if reinsertion_share is not None:
            bvh_builder |= int(reinsertion_share) << 16
        if presplit is not None:
            bvh_builder |= min(int(presplit), 127) << 24
        if path is not None:
            rc = lib().tb_host_scene_load(os.fsencode(path), bvh_builder, (1 if flatten_instances else 0) | (0 if flip_texture_uvs else 2), C.byref(self._h), err, 512)
        else:
            kind, tris, seed = procedural
            rc = lib().tb_host_scene_procedural(kind, tris, seed, bvh_builder, C.byref(self._h), err, 512)
        if rc != 0:
            raise TracerBoyError(rc, err.value.decode(errors="replace"))

    @classmethod
    def from_meshes(cls, meshes, materials, camera=None, environment=None, env_scale=(1, 1, 1), film=(0, 0), bvh_builder=0):
        """tb_host_scene_from_meshes: the host half of TracerBoy.LoadMeshes (numpy arrays only)."""
        d, keep, _ = _scene_desc("HostScene.from_meshes", meshes, materials, camera, environment, env_scale, film, None)
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib().tb_host_scene_from_meshes(C.byref(d), bvh_builder, C.byref(self._h), err, 512)
        if rc != 0:
            raise TracerBoyError(rc, err.value.decode(errors="replace"))
        return self

    def close(self):
        if self._h:
            lib().tb_host_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def view(self):
        v = abi.TbSceneView()
        lib().tb_host_scene_view_get(self._h, C.byref(v))
        return v

    def camera(self):
        c = abi.tb_camera()
        lib().tb_host_scene_camera(self._h, C.byref(c))
        return c

    def info(self):
        i = abi.tb_scene_info()
        lib().tb_host_scene_info(self._h, C.byref(i))
        return i

    def frame_constants(self, settings=None, frame=0, time_seed=0.0):
        pf = abi.TbPerFrameConstants()
        lib().tb_host_scene_frame_constants(self._h, C.byref(settings) if settings is not None else None, frame, time_seed, C.byref(pf))
        return pf

    def digest(self):
        """The scene digest a context reports for this scene and builder (tb_host_scene_digest)."""
        d = C.c_uint64()
        rc = lib().tb_host_scene_digest(self._h, C.byref(d))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_digest")
        return d.value

    def bvh_bytes(self):
        v = self.view()
        return np.ctypeslib.as_array(C.cast(v.bvh, C.POINTER(C.c_uint8)), shape=(v.bvhBytes,)).copy()

    def triangles(self):
        pos = C.POINTER(C.c_float)(); nv = C.c_uint32(); tvi = C.POINTER(C.c_uint32)(); tg = C.POINTER(C.c_uint32)()
        tp = C.POINTER(C.c_uint32)(); tf = C.POINTER(C.c_uint32)(); nt = C.c_uint32()
        lib().tb_host_scene_triangles(self._h, C.byref(pos), C.byref(nv), C.byref(tvi), C.byref(tg), C.byref(tp), C.byref(tf), C.byref(nt))
        n, m = nt.value, nv.value
        return dict(positions=np.ctypeslib.as_array(pos, shape=(m, 3)).copy(), tri_vertex_index=np.ctypeslib.as_array(tvi, shape=(n, 3)).copy(),
                    tri_geometry=np.ctypeslib.as_array(tg, shape=(n,)).copy(), tri_primitive=np.ctypeslib.as_array(tp, shape=(n,)).copy(),
                    tri_flags=np.ctypeslib.as_array(tf, shape=(n,)).copy())

    def layout_b(self):
        nodes = C.POINTER(abi.TbNodeB)(); nn = C.c_uint32(); tris = C.POINTER(abi.TbTriB)(); nt = C.c_uint32(); root = C.c_uint32()
        lib().tb_host_scene_layout_b(self._h, C.byref(nodes), C.byref(nn), C.byref(tris), C.byref(nt), C.byref(root))
        nb = np.frombuffer(C.string_at(nodes, nn.value * 64), dtype=np.uint32).reshape(nn.value, 16).copy()
        tb = np.frombuffer(C.string_at(tris, nt.value * 48), dtype=np.uint32).reshape(nt.value, 12).copy()
        return nb, tb, root.value

    def nearest(self, points, signed=False, walk=False):
        """tb_host_scene_nearest: the NEAREST_DTYPE records of include/tb_nearest.h's rule for QUERY_POINT_DTYPE (or float32 (n, 4)) points, by brute
        force over every triangle or, walk=True, by the kernel's walk and pruning rule as scalar C++."""
        _check_query_points("HostScene.nearest", points, 0, allow_tensor=False)
        flags = (NEAREST_SIGNED if _check_flag("HostScene.nearest", "signed", signed) else 0) | \
            (NEAREST_HOST_WALK if _check_flag("HostScene.nearest", "walk", walk) else NEAREST_HOST_BRUTE)
        out = np.empty(points.shape[0], NEAREST_DTYPE)
        rc = lib().tb_host_scene_nearest(self._h, flags, points.shape[0], _np_ptr(points), _np_ptr(out))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_nearest")
        return out

    def winding(self, points, beta=WINDING_BETA, walk=False):
        """tb_host_scene_winding: float32 (n,), include/tb_winding.h's winding number of the scene's triangles at QUERY_POINT_DTYPE (or float32
        (n, 4)) points -- the exact sum over every triangle in order or, walk=True, the kernel's walk with far subtrees as dipoles (beta=inf: none)."""
        _check_query_points("HostScene.winding", points, 0, allow_tensor=False)
        beta = _check_beta("HostScene.winding", beta)
        flags = WINDING_HOST_WALK if _check_flag("HostScene.winding", "walk", walk) else WINDING_HOST_BRUTE
        out = np.empty(points.shape[0], np.float32)
        rc = lib().tb_host_scene_winding(self._h, flags, points.shape[0], _np_ptr(points), beta, _np_ptr(out))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_winding")
        return out

    def nearest_excess(self, points):
        """tb_host_scene_nearest_excess: the largest sqrt(box d2) - sqrt(D2) over the boxes above a brute-force winner, in 2^-23 x the scale."""
        _check_query_points("HostScene.nearest_excess", points, 0, allow_tensor=False)
        worst = C.c_float()
        rc = lib().tb_host_scene_nearest_excess(self._h, points.shape[0], _np_ptr(points), C.byref(worst))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_nearest_excess")
        return worst.value

    def lds_image(self):
        """(image bytes as uint8, tb_lds_image_info): the walk's LDS image as a context uploads it for an LDS-resident scene."""
        info = abi.tb_lds_image_info()
        rc = lib().tb_host_scene_lds_image(self._h, None, 0, C.byref(info))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_lds_image")
        buf = np.zeros(info.bytes, dtype=np.uint8)
        rc = lib().tb_host_scene_lds_image(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), info.bytes, C.byref(info))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_lds_image")
        return buf, info

    # ---- what a wave pays for the tree (csrc/host/wave_cost.h) ----
    def wave_stage(self):
        """tb_wave_stage_info: what builder 1's wave stage did when this scene was built (ran = 0: it did not run)."""
        info = abi.tb_wave_stage_info()
        rc = lib().tb_host_scene_wave_stage(self._h, C.byref(info))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_wave_stage")
        return info

    def wave_search(self, seed=0, waves=0, feeler_percent=-1, places=0, keep=0, threads=0):
        """Builds this scene's tree again with builder 1 and the wave stage on (tb_host_scene_wave_search) and returns its tb_wave_stage_info: the
        stage's model rays from seed / waves / feeler_percent (0 / 0 / -1: its own), `places` per cut subtree (0 = every legal place, 3 = the three
        best by induced area: the stage as it was before it priced them all), `keep` places of a cut from the screen to all waves (0 = the stage's
        own, a number no cut reaches = no screen), `threads` workers (0 = the library's choice, 1 = serial)."""
        info = abi.tb_wave_stage_info()
        rc = lib().tb_host_scene_wave_search(self._h, seed, waves, feeler_percent, places, keep, threads, C.byref(info))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_wave_search")
        return info

    def wave_rays(self, seed=0, waves=0, feeler_percent=-1):
        """(origins, dirs, t_max) of the wave stage's model rays for this scene; 0 / 0 / -1: the stage's own seed, size and feeler share."""
        fp = C.POINTER(C.c_float)
        n = lib().tb_host_scene_wave_rays(self._h, seed, waves, feeler_percent, None, None, None, 0)
        if n < 0:
            raise TracerBoyError(n, "tb_host_scene_wave_rays")
        o = np.zeros((n, 3), dtype=np.float32); d = np.zeros((n, 3), dtype=np.float32); t = np.zeros(n, dtype=np.float32)
        lib().tb_host_scene_wave_rays(self._h, seed, waves, feeler_percent, o.ctypes.data_as(fp), d.ctypes.data_as(fp), t.ctypes.data_as(fp), n)
        return o, d, t

    def wave_walk(self, origins, dirs, t_max=None, want_steps=False):
        """The single-ray walk of wave_cost.h over this scene's tree: (inner steps, leaf steps[, step strings]) per ray."""
        fp = C.POINTER(C.c_float); up = C.POINTER(C.c_uint32)
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3); d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        t = None if t_max is None else np.ascontiguousarray(t_max, dtype=np.float32)
        n = len(o); inner = np.zeros(n, dtype=np.uint32); leaf = np.zeros(n, dtype=np.uint32)
        rc = lib().tb_host_scene_wave_walk(self._h, n, o.ctypes.data_as(fp), d.ctypes.data_as(fp), None if t is None else t.ctypes.data_as(fp),
                                           inner.ctypes.data_as(up), leaf.ctypes.data_as(up), None, 0)
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_wave_walk")
        if not want_steps:
            return inner, leaf
        cap = int(inner.sum()) + int(leaf.sum()) + n
        buf = C.create_string_buffer(cap)
        rc = lib().tb_host_scene_wave_walk(self._h, n, o.ctypes.data_as(fp), d.ctypes.data_as(fp), None if t is None else t.ctypes.data_as(fp), None, None, buf, cap)
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_wave_walk")
        return inner, leaf, [w.decode() for w in buf.raw[:cap].split(b"\0")[:n]]

    def wave_cost(self, seed=0, waves=0, feeler_percent=-1, park_min=0):
        """tb_wave_trips of the model rays over this scene's tree."""
        out = abi.tb_wave_trips()
        rc = lib().tb_host_scene_wave_cost(self._h, seed, waves, feeler_percent, park_min, C.byref(out))
        if rc != 0:
            raise TracerBoyError(rc, "tb_host_scene_wave_cost")
        return out


def wave_replay(steps, park_min=2):
    """tb_wave_trips of up to 64 step strings of 'I' / 'L' replayed in lock step under the LDS-resident walk's schedule (tb_wave_replay)."""
    arr = (C.c_char_p * max(len(steps), 1))(*[s.encode() for s in steps])
    out = abi.tb_wave_trips()
    rc = lib().tb_wave_replay(arr, len(steps), park_min, C.byref(out))
    if rc != 0:
        raise TracerBoyError(rc, "tb_wave_replay")
    return out


class TracerBoy:
    """Drop-in for the hot-path surface of the reference's `class TracerBoy` on one MI355X."""

    def __init__(self, device_id=0, devices=None):
        """device_id: one HIP device.  devices=[...]: ONE object driving several devices of this process (tb_create_multi): the frame's
        tiles are dealt over them, gathered peer-to-peer and assembled on devices[0]."""
        self._L = lib()
        self._ctx = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._L.tb_create_multi(C.byref(self._ctx), ids, len(devices))
        else:
            rc = self._L.tb_create(C.byref(self._ctx), int(device_id))
        if rc != 0:
            raise TracerBoyError(rc, (self._L.tb_last_error(None) or b"").decode(errors="replace"))
        self.width = self.height = 0
        self._budget_shape = None
        self._device = int(devices[0]) if devices is not None else int(device_id)

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.tb_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise TracerBoyError(rc, (self._L.tb_last_error(self._ctx) or b"").decode(errors="replace"))

    def _query(self, on_device, device_flag, call, tensor_shape, array_shape, dtype=np.float32, out=None):
        """The tail of every query method, after its checks.  call(flag, ptr, o) is the entry point: ptr(a) makes the pointer of one of its
        arrays, o is the result's.  The host path -- flag = 0 -- answers in a numpy array of array_shape and dtype.  The device path -- flag =
        device_flag -- answers in a torch tensor of tensor_shape on the context's device, after torch's work there is done: bytes where dtype is
        np.uint8, else float32, a record's fields as columns.  out: the caller's own result array, already checked, in place of a new one."""
        if on_device:
            import torch
            dev = torch.device("cuda", getattr(self, "_device", 0))
            if out is None:
                out = torch.empty(tensor_shape, dtype=torch.uint8 if dtype is np.uint8 else torch.float32, device=dev)
            _torch_sync(dev)
            self._check(call(device_flag, _tensor_ptr, _tensor_ptr(out)))
        else:
            if out is None:
                out = np.empty(array_shape, dtype)
            self._check(call(0, _np_ptr, _np_ptr(out)))
        return out

    # -- TracerBoy interface --------------------------------------------------------------------
    def LoadScene(self, sceneFileName):
        """TracerBoy::LoadScene (TracerBoy.cpp:1065): blocking."""
        self._num_vertices = None
        self._check(self._L.tb_load_scene(self._ctx, os.fsencode(sceneFileName)))

    def LoadProcedural(self, kind, target_triangles, seed=1234):
        self._num_vertices = None
        self._check(self._L.tb_load_procedural(self._ctx, kind, target_triangles, seed))

    def LoadMeshes(self, meshes, materials, camera=None, environment=None, env_scale=(1, 1, 1), film=(0, 0)):
        """tb_load_meshes: a scene from api.Mesh objects and TbMaterials instead of a file.  Arrays: numpy, or contiguous torch
        tensors on the context's device (read to the host once).  Wrong arrays: ValueError, before any library call."""
        meshes = list(meshes)
        d, keep, on_device = _scene_desc("LoadMeshes", meshes, materials, camera, environment, env_scale, film, getattr(self, "_device", 0))
        if on_device:
            _torch_sync(meshes[0].positions.device)
        self._num_vertices = None
        self._check(self._L.tb_load_meshes(self._ctx, C.byref(d)))

    def Render(self, width, height, n_frames=1, outputSettings=None, time_seed=0.0, sync=True):
        """TracerBoy::Render x n_frames (TracerBoy.cpp:2677); one sample per pixel per frame."""
        fn = self._L.tb_render if sync else self._L.tb_render_async
        self._check(fn(self._ctx, width, height, n_frames, C.byref(outputSettings) if outputSettings is not None else None, time_seed))
        self.width, self.height = width, height

    def Sync(self):
        self._check(self._L.tb_sync(self._ctx))

    def GetNumberOfSamplesSinceLastInvalidate(self):
        return int(self._L.tb_samples_rendered(self._ctx))

    def InvalidateHistory(self):
        self._L.tb_invalidate_history(self._ctx)

    def GetCamera(self):
        c = abi.tb_camera()
        self._check(self._L.tb_get_camera(self._ctx, C.byref(c)))
        return c

    def SetCamera(self, cam):
        self._check(self._L.tb_set_camera(self._ctx, C.byref(cam)))

    def IsMaterialIDValid(self, i):
        return 0 <= i < self._L.tb_material_count(self._ctx)

    def GetMaterial(self, i):
        m = abi.TbMaterial()
        self._check(self._L.tb_get_material(self._ctx, i, C.byref(m)))
        return m

    def SetMaterial(self, i, m):
        self._check(self._L.tb_set_material(self._ctx, i, C.byref(m)))

    def SelectPixel(self, x, y):
        self._check(self._L.tb_select_pixel(self._ctx, x, y))

    def ReadbackStats(self):
        s = abi.tb_readback_stats()
        self._check(self._L.tb_read_stats(self._ctx, C.byref(s)))
        return s

    def WaveProfile(self):
        """Per-phase wave occupancy of the last counting render: {phase: (active_lanes, trips, occupancy)}."""
        raw = (C.c_uint64 * 14)()
        self._check(self._L.tb_read_wave_profile(self._ctx, raw))
        names = ["bvh_inner", "bvh_leaf", "closest_shade", "shadow_slot", "scatter", "regenerate", "iteration"]
        return {n: (int(raw[2 * i]), int(raw[2 * i + 1]), (raw[2 * i] / (64.0 * raw[2 * i + 1])) if raw[2 * i + 1] else 0.0) for i, n in enumerate(names)}

    def SplitProfile(self):
        """Counters of the split-role kernel (pipeline 4 rendered with option split_profile = 1), with the ratios that matter."""
        raw = (C.c_uint64 * 16)()
        self._check(self._L.tb_read_split_profile(self._ctx, raw))
        v = [int(x) for x in raw]
        d = dict(t_inner_steps=v[0], t_inner_lanes=v[1], t_leaf_steps=v[2], t_leaf_lanes=v[3], t_ticket_draws=v[4], t_rays=v[5], t_sleeps=v[6], t_cycles=v[7],
                 s_rounds=v[8], s_lanes=v[9], s_sleeps=v[10], s_cycles=v[11], s_rays=v[12], s_samples=v[13], t_waves=v[14], s_waves=v[15])
        d["inner_occupancy"] = v[1] / (64.0 * v[0]) if v[0] else 0.0
        d["leaf_occupancy"] = v[3] / (64.0 * v[2]) if v[2] else 0.0
        d["shade_occupancy"] = v[9] / (64.0 * v[8]) if v[8] else 0.0
        d["cycles_per_walk_step"] = v[7] / float(v[0] + v[2]) if v[0] + v[2] else 0.0
        return d

    # -- surfaces -------------------------------------------------------------------------------
    def ReadAccumulation(self, jittered=False):
        """(H, W, 4) float32 sums (rgb*w, w) of OutputTexture (and JitteredOutputTexture)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        jit = np.empty_like(out) if jittered else None
        self._check(self._L.tb_read_accum(self._ctx, _np_ptr(out), _np_ptr(jit) if jittered else None))
        return (out, jit) if jittered else out

    # -- render states ----------------------------------------------------
    def BeginAccumulation(self, width, height, outputSettings=None, time_seed=0.0, first_frame=0):
        """The context holds the empty state [first_frame, first_frame): the next Render with the same size, settings and time seed renders
        frames first_frame, first_frame + 1, ... onto zeroed surfaces (tb_state_begin)."""
        self._check(self._L.tb_state_begin(self._ctx, width, height, C.byref(outputSettings) if outputSettings is not None else None, time_seed, first_frame))
        self.width, self.height = width, height

    def SaveState(self, path):
        """Surfaces, frame range, settings, camera, tile assignment and digests into one file, atomically (tb_state_save)."""
        self._check(self._L.tb_state_save(self._ctx, os.fsencode(path)))

    def LoadState(self, path, add=False, any_scene=False):
        """add=False: the context becomes the file's state and a following Render continues it bit for bit.  add=True: the file's sums are added
        to the context's (adjacent frame ranges; the fp32 sum of the partial sums).  any_scene: do not compare the scene digests."""
        flags = (TB_STATE_ADD if add else TB_STATE_REPLACE) | (TB_STATE_ANY_SCENE if any_scene else 0)
        self._check(self._L.tb_state_load(self._ctx, os.fsencode(path), flags))
        if not add:
            info = StateInfo(path)
            self.width, self.height = info.width, info.height

    def AccumDigest(self):
        """(output digest, jittered digest) computed on the device from the surfaces as they lie in HBM (tb_accum_digest)."""
        d = (C.c_uint64 * 2)()
        self._check(self._L.tb_accum_digest(self._ctx, d))
        return int(d[0]), int(d[1])

    def SceneDigest(self):
        d = C.c_uint64()
        self._check(self._L.tb_scene_digest(self._ctx, C.byref(d)))
        return d.value

    def RenderRealTime(self, width, height, outputSettings=None, denoiserSettings=None, time_seed=0.0):
        """One displayed frame of RenderMode::RealTime: 1 spp + TAA + a-trous denoiser + albedo composite + TAA (TracerBoy.cpp:2677-3160)."""
        self._check(self._L.tb_render_realtime(self._ctx, width, height, C.byref(outputSettings) if outputSettings is not None else None,
                                               C.byref(denoiserSettings) if denoiserSettings is not None else None, time_seed))
        self.width, self.height = width, height

    def ReadRealTimeStage(self, stage):
        """0 first TAA output (rgb, variance), 1 moments, 2 denoised, 3 composited, 4 final TAA output."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.tb_read_realtime(self._ctx, stage, _np_ptr(out)))
        return out

    def Denoise(self, denoiserSettings=None, read=True):
        """Denoise the progressive render the context holds (tb_denoise): dual-buffer variance, 3x3 prefilter,
        WaveletIterations a-trous passes guided by the AOVs of the last frame (render with option "aov"), (rgb, 1).  Leaves the accumulation as
        it is.  Returns the (H, W, 4) float32 result, or None with read=False (ReadDenoiseStage(3), or option "post_denoised" + PostProcess)."""
        out = np.empty((self.height, self.width, 4), np.float32) if read else None
        self._check(self._L.tb_denoise(self._ctx, C.byref(denoiserSettings) if denoiserSettings is not None else None, _np_ptr(out) if read else None))
        return out

    def ReadDenoiseStage(self, stage):
        """0 prepared (mean rgb, variance), 1 filtered (variance after the 3x3 Gaussian), 2 the last filter pass's output, 3 final (rgb, 1)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.tb_read_denoise_stage(self._ctx, stage, _np_ptr(out)))
        return out

    def RenderGuides(self, first_frame, n_frames):
        """The guide pass (tb_render_guides): the first hits of frames [first_frame, first_frame + n_frames) traced again with
        the context's current size, settings, time seed and camera, summed into the three guide surfaces.  Leaves everything else as it is.
        Option "denoise_guides" = 1 / 2 makes Denoise read them."""
        self._check(self._L.tb_render_guides(self._ctx, first_frame, n_frames))

    def ReadGuide(self, which):
        """0 albedo (sum of the effective albedo, frames), 1 normal (sum over the frames that hit, their number), 2 position (sum of world
        positions, sum of neighbour distances): (H, W, 4) float32."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._L.tb_read_guide(self._ctx, which, _np_ptr(out)))
        return out

    # -- the path inspector ------------------------------------------------
    def RecordPaths(self, x, y, first_frame, n_frames):
        """The complete paths of pixel (x, y) traced again for frames [first_frame, first_frame + n_frames) (tb_record_paths): their bounce rays are
        appended to the ray buffer.  Returns (frames, rays_total): a structured array (PATH_FRAME_DTYPE) with one record per frame -- what the
        render adds to the output surface for that sample, where its rays lie, flags -- and the rays the call would have stored without the cap."""
        frames, total = np.zeros(n_frames, PATH_FRAME_DTYPE), C.c_uint32(0)
        self._check(self._L.tb_record_paths(self._ctx, x, y, first_frame, n_frames, _np_ptr(frames), C.byref(total)))
        return frames, int(total.value)

    def ReadPaths(self):
        """The ray buffer (tb_read_paths): a structured array (VISUALIZER_RAY_DTYPE) of the stored rays, frame by frame, bounce by bounce."""
        n = C.c_uint32(0)
        self._check(self._L.tb_read_paths(self._ctx, None, 0, C.byref(n)))
        rays = np.zeros(n.value, VISUALIZER_RAY_DTYPE)
        if n.value:
            self._check(self._L.tb_read_paths(self._ctx, _np_ptr(rays), n.value, C.byref(n)))
        return rays

    def ClearPaths(self):
        self._check(self._L.tb_clear_paths(self._ctx))

    def VisualizeRays(self, settings=None, rgba8=True):
        """The stored rays drawn over the float picture of the last PostProcess (tb_visualize_rays, VisualizeRaysCS.hlsl): returns (float32 HxWx4
        image, uint8 HxWx4 image or None).  The post output itself is not modified."""
        f = np.empty((self.height, self.width, 4), np.float32)
        b = np.empty((self.height, self.width, 4), np.uint8) if rgba8 else None
        self._check(self._L.tb_visualize_rays(self._ctx, C.byref(settings) if settings is not None else None, _np_ptr(f), _np_ptr(b) if rgba8 else None))
        return f, b

    def RunVisualizeRays(self, constants, rays, scene, world_pos=None):
        """vis_overlay on host arrays (tb_run_visualize_rays): rays a VISUALIZER_RAY_DTYPE array (or (n, 8) float32), scene and world_pos (H, W, 4)
        float32 with H, W from the constants; nothing of the context read or written."""
        r = np.ascontiguousarray(rays); s = np.ascontiguousarray(scene, np.float32)
        w = None if world_pos is None else np.ascontiguousarray(world_pos, np.float32)
        assert r.nbytes % 32 == 0 and s.shape == (constants.ResolutionY, constants.ResolutionX, 4) and (w is None or w.shape == s.shape)
        out = np.empty_like(s)
        self._check(self._L.tb_run_visualize_rays(self._ctx, C.byref(constants), _np_ptr(r) if r.nbytes else None, r.nbytes // 32, _np_ptr(s),
                                                  _np_ptr(w) if w is not None else None, _np_ptr(out)))
        return out

    def PostProcess(self, postSettings=None, outputType=0, rgba8=True):
        """The tail of TracerBoy::Render (TracerBoy.cpp:2948-3200): auto exposure + PostProcessCS on the surface the output
        type selects.  Returns (float32 HxWx4 image, uint8 HxWx4 back-buffer image or None)."""
        ps = postSettings if postSettings is not None else GetDefaultPostProcessSettings()
        f = np.empty((self.height, self.width, 4), np.float32)
        b = np.empty((self.height, self.width, 4), np.uint8) if rgba8 else None
        self._check(self._L.tb_post_process(self._ctx, C.byref(ps), outputType, _np_ptr(f), _np_ptr(b) if rgba8 else None))
        return f, b

    def Upscale(self, out_width, out_height, postSettings=None, outputType=0, sharpness=-1.0, rgba8=True):
        """PostProcess at the rendered size, then FSR 1 (EASU -> RCAS) to out_width x out_height (tb_upscale); sharpness in
        stops, negative = the reference's 0.2.  Returns (float32 image of the RGBA32F chain, uint8 image of the R8G8B8A8_UNORM chain or None),
        both out_height x out_width x 4."""
        ps = postSettings if postSettings is not None else GetDefaultPostProcessSettings()
        f = np.empty((out_height, out_width, 4), np.float32)
        b = np.empty((out_height, out_width, 4), np.uint8) if rgba8 else None
        self._check(self._L.tb_upscale(self._ctx, C.byref(ps), outputType, out_width, out_height, sharpness, _np_ptr(f), _np_ptr(b) if rgba8 else None))
        return f, b

    def LoadNeuralWeights(self, path):
        """Read a TZA weights file of the neural still denoiser, repack it for the kernel and upload it (tb_neural_load);
        replaces weights loaded before.  Option "neural_inputs" tells 3 or 9 afterwards."""
        self._check(self._L.tb_neural_load(self._ctx, os.fsencode(path)))

    def RunConv3x3(self, in_a, weight, bias, in_b=None, upsample_a=False, pool=False, relu=True):
        """One layer at the layer seam (tb_run_conv3x3): in_a (H, W, c_a) -- (H / 2, W / 2, c_a) with upsample_a -- and in_b (H, W, c_b) or None,
        weight (c_out, c_a + c_b, 3, 3), bias (c_out,), all float16.  Returns (H, W, c_out) float16, (H / 2, W / 2, c_out) with pool."""
        a = np.ascontiguousarray(in_a, np.float16); b = None if in_b is None else np.ascontiguousarray(in_b, np.float16)
        w = np.ascontiguousarray(weight, np.float16); bi = np.ascontiguousarray(bias, np.float16)
        H, W = (a.shape[0] * 2, a.shape[1] * 2) if upsample_a else a.shape[:2]
        if b is not None: H, W = b.shape[:2]
        c_b = 0 if b is None else b.shape[2]
        assert w.shape == (w.shape[0], a.shape[2] + c_b, 3, 3) and bi.shape == (w.shape[0],), "weight is (c_out, c_a + c_b, 3, 3), bias (c_out,)"
        d = abi.tb_conv3x3_desc(W, H, a.shape[2], c_b, w.shape[0], int(bool(upsample_a)), int(bool(pool)), int(bool(relu)))
        out = np.empty((H // 2, W // 2, w.shape[0]) if pool else (H, W, w.shape[0]), np.float16)
        self._check(self._L.tb_run_conv3x3(self._ctx, C.byref(d), _np_ptr(a), None if b is None else _np_ptr(b), _np_ptr(w), _np_ptr(bi), _np_ptr(out)))
        return out

    def RunNeural(self, color, albedo=None, normal=None):
        """The network on host surfaces (tb_run_neural): (H, W, 4) float32 each, .xyz read; albedo and normal exactly when the loaded weights have
        9 inputs.  Returns (H, W, 4) float32, alpha 1."""
        f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (color, albedo, normal)]
        h, w = f[0].shape[:2]
        assert all(a is None or a.shape == (h, w, 4) for a in f), "surfaces are (H, W, 4)"
        out = np.empty((h, w, 4), np.float32)
        self._check(self._L.tb_run_neural(self._ctx, w, h, *[None if a is None else _np_ptr(a) for a in f], _np_ptr(out)))
        return out

    def DenoiseNeural(self, postSettings=None, rgba8=True):
        """PostProcess at the rendered size, then the network on its 8-bit picture (each channel k / 255, as the reference's network reads it) and,
        with 9-input weights, on the albedo and normals of the guide pass (tb_denoise_neural; RenderGuides first).  Returns (float32 HxWx4 picture, uint8 HxWx4 picture or None)."""
        ps = postSettings if postSettings is not None else GetDefaultPostProcessSettings()
        f = np.empty((self.height, self.width, 4), np.float32)
        b = np.empty((self.height, self.width, 4), np.uint8) if rgba8 else None
        self._check(self._L.tb_denoise_neural(self._ctx, C.byref(ps), _np_ptr(f), _np_ptr(b) if rgba8 else None))
        return f, b

    def LoadUpscaleWeights(self, path):
        """Read a weights file of the neural 2 x super-resolution, fold and repack it for the kernel and upload it (tb_sr_load, DESIGN.md section
        16); replaces weights loaded before.  Option "sr_loaded" is 1 afterwards."""
        self._check(self._L.tb_sr_load(self._ctx, os.fsencode(path)))

    def RunConv(self, in_a, weight, bias=None, in_b=None, upsample_a=False, relu=True, form=0):
        """One layer at the layer seam (tb_run_conv): in_a (H, W, c_a) -- (H / 2, W / 2, c_a) with upsample_a -- and in_b (H, W, c_b) or None,
        weight (c_out, c_a + c_b, K, K) with K 3 or 5, bias (c_out,) or None, all float16.  Returns (H, W, c_out) float16."""
        a = np.ascontiguousarray(in_a, np.float16); b = None if in_b is None else np.ascontiguousarray(in_b, np.float16)
        w = np.ascontiguousarray(weight, np.float16); bi = None if bias is None else np.ascontiguousarray(bias, np.float16)
        H, W = (a.shape[0] * 2, a.shape[1] * 2) if upsample_a else a.shape[:2]
        if b is not None: H, W = b.shape[:2]
        c_b = 0 if b is None else b.shape[2]
        assert w.ndim == 4 and w.shape[1] == a.shape[2] + c_b and w.shape[2] == w.shape[3], "weight is (c_out, c_a + c_b, K, K)"
        assert bi is None or bi.shape == (w.shape[0],), "bias is (c_out,)"
        d = abi.tb_conv_desc(W, H, a.shape[2], c_b, w.shape[0], w.shape[2], int(bool(upsample_a)), int(bool(relu)), form)
        out = np.empty((H, W, w.shape[0]), np.float16)
        self._check(self._L.tb_run_conv(self._ctx, C.byref(d), _np_ptr(a), None if b is None else _np_ptr(b), _np_ptr(w), None if bi is None else _np_ptr(bi),
                                        _np_ptr(out)))
        return out

    def RunSrFinish(self, residual, picture):
        """The network's residual add (tb_run_sr_finish): residual (2 H, 2 W, 3) and picture (H, W, 3) float16.  Returns (2 H, 2 W, 4) float32:
        |half(residual + picture nearest-upsampled x 2)| and alpha 1."""
        r, p = np.ascontiguousarray(residual, np.float16), np.ascontiguousarray(picture, np.float16)
        h, w = p.shape[:2]
        assert p.shape == (h, w, 3) and r.shape == (2 * h, 2 * w, 3), "residual is (2 H, 2 W, 3), picture (H, W, 3)"
        out = np.empty((2 * h, 2 * w, 4), np.float32)
        self._check(self._L.tb_run_sr_finish(self._ctx, w, h, _np_ptr(r), _np_ptr(p), _np_ptr(out)))
        return out

    def RunUpscaleNeural(self, color):
        """The super-resolution network on a host surface (tb_run_sr): (H, W, 4) float32, .xyz read.  Returns (2 H, 2 W, 4) float32, alpha 1."""
        f = np.ascontiguousarray(color, np.float32)
        h, w = f.shape[:2]
        assert f.shape == (h, w, 4), "the surface is (H, W, 4)"
        out = np.empty((2 * h, 2 * w, 4), np.float32)
        self._check(self._L.tb_run_sr(self._ctx, w, h, _np_ptr(f), _np_ptr(out)))
        return out

    def UpscaleNeural(self, postSettings=None, rgba8=True):
        """PostProcess at the rendered size, then the super-resolution network on its 8-bit picture (each channel k / 255, as the reference's network
        reads it; tb_upscale_neural).  Returns (float32 2Hx2Wx4 picture, uint8 2Hx2Wx4 picture or None)."""
        ps = postSettings if postSettings is not None else GetDefaultPostProcessSettings()
        f = np.empty((2 * self.height, 2 * self.width, 4), np.float32)
        b = np.empty((2 * self.height, 2 * self.width, 4), np.uint8) if rgba8 else None
        self._check(self._L.tb_upscale_neural(self._ctx, C.byref(ps), _np_ptr(f), _np_ptr(b) if rgba8 else None))
        return f, b

    def RunNnPack(self, color, albedo=None, normal=None, unorm_color=False):
        """nn_pack_input on host surfaces (tb_run_nn_pack): (H, W, 4) float32 each, albedo and normal both or neither.  Returns the network's input,
        (H0, W0, 32) float16 with H0, W0 the next multiples of 16.  unorm_color: the colour goes through the 8-bit store, as in the stage."""
        f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (color, albedo, normal)]
        h, w = f[0].shape[:2]
        assert all(a is None or a.shape == (h, w, 4) for a in f), "surfaces are (H, W, 4)"
        out = np.empty((h + -h % 16, w + -w % 16, 32), np.float16)
        self._check(self._L.tb_run_nn_pack(self._ctx, w, h, out.shape[1], out.shape[0], int(bool(unorm_color)), *[None if a is None else _np_ptr(a) for a in f],
                                           _np_ptr(out)))
        return out

    def RunNnUnpack(self, tensor, width, height):
        """nn_unpack_output on a host tensor (tb_run_nn_unpack): (H0, W0, 32) float16 -> (height, width, 4) float32, channels 0-2 and alpha 1."""
        t = np.ascontiguousarray(tensor, np.float16)
        assert t.ndim == 3 and t.shape[2] == 32, "the tensor is (H0, W0, 32)"
        out = np.empty((height, width, 4), np.float32)
        self._check(self._L.tb_run_nn_unpack(self._ctx, width, height, t.shape[1], t.shape[0], _np_ptr(t), _np_ptr(out)))
        return out

    def RunNnResolveAux(self, albedo_sum, normal_sum):
        """nn_resolve_aux on host copies of the albedo and normal guide sums (tb_run_nn_resolve_aux), (H, W, 4) float32 each.  Returns (albedo,
        normal) as the network's pack reads them."""
        a, n = np.ascontiguousarray(albedo_sum, np.float32), np.ascontiguousarray(normal_sum, np.float32)
        h, w = a.shape[:2]
        assert a.shape == n.shape == (h, w, 4), "surfaces are (H, W, 4)"
        albedo, normal = np.empty_like(a), np.empty_like(a)
        self._check(self._L.tb_run_nn_resolve_aux(self._ctx, w, h, _np_ptr(a), _np_ptr(n), _np_ptr(albedo), _np_ptr(normal)))
        return albedo, normal

    def RunNnToRgba8(self, image):
        """nn_to_rgba8 on a host surface (tb_run_nn_to_rgba8): (H, W, 4) float32 -> (H, W, 4) uint8."""
        a = np.ascontiguousarray(image, np.float32)
        h, w = a.shape[:2]
        assert a.shape == (h, w, 4), "the surface is (H, W, 4)"
        out = np.empty((h, w, 4), np.uint8)
        self._check(self._L.tb_run_nn_to_rgba8(self._ctx, w, h, _np_ptr(a), _np_ptr(out)))
        return out

    @staticmethod
    def _fsr_surface(image):
        """(surface type, contiguous array) of an (H, W, 4) image: uint8 = R8G8B8A8_UNORM, anything else = RGBA32F."""
        if np.asarray(image).dtype == np.uint8:
            return abi.TB_FSR_SURFACE_UNORM8, np.ascontiguousarray(image, np.uint8)
        return abi.TB_FSR_SURFACE_F32, np.ascontiguousarray(image, np.float32)

    def RunFsrEasu(self, constants, image, out_width, out_height):
        """fsr_easu_kernel on a host image (H, W, 4), uint8 or float32 (the surface type follows the dtype); nothing of the context read or written."""
        surface, a = self._fsr_surface(image)
        out = np.empty((out_height, out_width, 4), a.dtype)
        self._check(self._L.tb_run_fsr_easu(self._ctx, C.byref(constants), surface, a.shape[1], a.shape[0], out_width, out_height, _np_ptr(a), _np_ptr(out)))
        return out

    def RunFsrRcas(self, constants, image):
        """fsr_rcas_kernel on a host image (H, W, 4), uint8 or float32."""
        surface, a = self._fsr_surface(image)
        out = np.empty_like(a)
        self._check(self._L.tb_run_fsr_rcas(self._ctx, C.byref(constants), surface, a.shape[1], a.shape[0], _np_ptr(a), _np_ptr(out)))
        return out

    # -- image-quality metrics --------------------------------------------
    @staticmethod
    def _compare_maps(width, height, maps):
        """(squared-error map, SSIM map) to hand to the library, or (None, None); the SSIM map is (H - 10, W - 10), empty without a window."""
        if not maps:
            return None, None
        return np.zeros((height, width), np.float32), np.zeros((max(height - 10, 0), max(width - 10, 0)), np.float32)

    @staticmethod
    def _compare_dict(result, sq, ssim):
        d = {n: getattr(result, n) for n in COMPARE_FIELDS}
        if sq is not None:
            d["sq_err_map"], d["ssim_map"] = sq, ssim
        return d

    def RunCompare(self, test, ref, settings=None, maps=False):
        """cmp_pointwise / cmp_ssim / cmp_finish on two host images (H, W, 4) float32 (tb_run_compare); nothing of the context read or written.
        settings.flags | TB_COMPARE_SUMS: test holds sums (rgb * w, w).  Returns a dict of tb_compare_result's fields; with maps=True also
        "sq_err_map" (H, W) and "ssim_map" (H - 10, W - 10)."""
        a, r = np.ascontiguousarray(test, np.float32), np.ascontiguousarray(ref, np.float32)
        if a.ndim != 3 or a.shape[2] != 4 or a.shape != r.shape:
            raise ValueError("RunCompare: two (H, W, 4) images of one size")
        out = abi.tb_compare_result()
        sq, ssim = self._compare_maps(a.shape[1], a.shape[0], maps)
        self._check(self._L.tb_run_compare(self._ctx, a.shape[1], a.shape[0], _np_ptr(a), _np_ptr(r), C.byref(settings) if settings is not None else None,
                                           C.byref(out), _np_ptr(sq) if maps else None, _np_ptr(ssim) if maps and ssim.size else None))
        return self._compare_dict(out, sq, ssim)

    def SetReference(self, image):
        """Upload the (H, W, 4) float32 reference picture Compare measures against, or release it with None (tb_set_reference)."""
        if image is None:
            self._check(self._L.tb_set_reference(self._ctx, 0, 0, None))
            return
        r = np.ascontiguousarray(image, np.float32)
        if r.ndim != 3 or r.shape[2] != 4:
            raise ValueError("SetReference: an (H, W, 4) image")
        self._check(self._L.tb_set_reference(self._ctx, r.shape[1], r.shape[0], _np_ptr(r)))

    def Compare(self, surface=0, settings=None, maps=False):
        """The metrics of the accumulation's mean (surface 0) or the denoised still (1) against the reference, on the device (tb_compare).
        Returns what RunCompare returns."""
        out = abi.tb_compare_result()
        sq, ssim = self._compare_maps(self.width, self.height, maps)
        self._check(self._L.tb_compare(self._ctx, surface, C.byref(settings) if settings is not None else None, C.byref(out),
                                       _np_ptr(sq) if maps else None, _np_ptr(ssim) if maps and ssim.size else None))
        return self._compare_dict(out, sq, ssim)

    def AveragedLuminance(self):
        v = C.c_float()
        self._check(self._L.tb_read_averaged_luminance(self._ctx, C.byref(v)))
        return v.value

    def ReadAOV(self, which):
        shape = (self.height, self.width) if which == 6 else (self.height, self.width, 4)
        out = np.empty(shape, np.float32)
        self._check(self._L.tb_read_aov(self._ctx, which, _np_ptr(out)))
        return out

    def AccumDevicePointers(self):
        o, j = C.c_void_p(), C.c_void_p()
        self._check(self._L.tb_accum_device_ptr(self._ctx, C.byref(o), C.byref(j)))
        return o.value, j.value

    # -- multi-GPU tiles --------------------------------------------------------------------------
    def SetTileAssignment(self, rank, world, tile_w=64, tile_h=64):
        self._check(self._L.tb_set_tile_assignment(self._ctx, rank, world, tile_w, tile_h))

    def OwnedPixels(self, width, height):
        return int(self._L.tb_owned_pixels(self._ctx, width, height))

    def PackOwnedTo(self, device_ptr, sync=True):
        fn = self._L.tb_pack_owned_device if sync else self._L.tb_pack_owned_device_async
        self._check(fn(self._ctx, C.c_void_p(device_ptr)))

    def UnpackGatheredTo(self, gathered_ptr, capacity_pixels, width, height, world, tile_w, tile_h, full_ptr, stream=0):
        """Rank 0: device-side un-permute of the gathered per-rank buffers into the full frame (tb_unpack_gathered_device)."""
        self._check(self._L.tb_unpack_gathered_device(self._ctx, C.c_void_p(stream or None), C.c_void_p(gathered_ptr), capacity_pixels, width, height, world, tile_w, tile_h, C.c_void_p(full_ptr)))

    def Stream(self):
        """the context's hipStream_t as an integer (torch.cuda.ExternalStream(tb.Stream()))"""
        return int(self._L.tb_stream(self._ctx) or 0)

    # -- misc -----------------------------------------------------------------------------------
    def SetOption(self, name, value):
        self._check(self._L.tb_set_option(self._ctx, name.encode(), int(value)))

    def GetOption(self, name):
        return int(self._L.tb_get_option(self._ctx, name.encode()))

    def LivePixels(self):
        """Option "last_live_pixels": the owned pixels that were live at the first frame of the last call (all owned pixels of a call that did not run the
        adaptive launch, option "adaptive").  Waits for the call."""
        return self.GetOption("last_live_pixels")

    def SceneInfo(self):
        i = abi.tb_scene_info()
        self._check(self._L.tb_scene_info_get(self._ctx, C.byref(i)))
        return i

    def HostSceneView(self):
        v = abi.TbSceneView()
        self._check(self._L.tb_host_scene_view(self._ctx, C.byref(v)))
        return v

    def FrameConstants(self, width, height, frame, settings=None, time_seed=0.0):
        pf = abi.TbPerFrameConstants()
        self._check(self._L.tb_make_frame_constants(self._ctx, width, height, frame, C.byref(settings) if settings is not None else None, time_seed, C.byref(pf)))
        return pf

    def LastRenderMs(self):
        return float(self._L.tb_last_render_ms(self._ctx))

    def TraceClosest(self, origins, dirs):
        o = np.ascontiguousarray(origins, np.float32); d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        r = dict(t=np.empty(n, np.float32), material=np.empty(n, np.int32), bary=np.empty((n, 2), np.float32), prim=np.empty(n, np.uint32),
                 geom=np.empty(n, np.uint32), normal=np.empty((n, 3), np.float32), uv=np.empty((n, 2), np.float32),
                 boxes=np.empty(n, np.uint32), tris=np.empty(n, np.uint32))
        self._check(self._L.tb_trace_closest(self._ctx, n, _np_ptr(o), _np_ptr(d), _np_ptr(r["t"]), _np_ptr(r["material"]), _np_ptr(r["bary"]),
                                             _np_ptr(r["prim"]), _np_ptr(r["geom"]), _np_ptr(r["normal"]), _np_ptr(r["uv"]), _np_ptr(r["boxes"]), _np_ptr(r["tris"])))
        return r

    def TraceRays(self, rays, mode=RAYS_CLOSEST):
        """tb_trace_rays: closest hits (RAYS_CLOSEST) or any-hit occlusion (RAYS_OCCLUDED) of the caller's rays.
        A numpy array -- QUERY_RAY_DTYPE (make_query_rays), or float32 of shape (n, 8): origin, TMax, direction, the flags' bits -- takes the host
        path and returns a QUERY_HIT_DTYPE array / a uint8 array.  A torch tensor, float32 (n, 8), contiguous, on the context's device, takes the
        device path with zero copy: torch's current stream on that device is synchronised first, and the result is a float32 (n, 12) tensor (the
        integer fields through .view(torch.int32)) / a uint8 (n,) tensor that torch allocated.  Anything else: ValueError, before any library call."""
        on_device = _check_query_rays(rays, mode, getattr(self, "_device", 0))
        n = int(rays.shape[0])
        closest = mode == RAYS_CLOSEST

        def call(dev, ptr, o):
            return self._L.tb_trace_rays(self._ctx, mode | dev, n, ptr(rays), o)
        return self._query(on_device, RAYS_DEVICE, call, (n, 12) if closest else (n,), n, QUERY_HIT_DTYPE if closest else np.uint8)

    # -- point queries ------------------------------------------------------
    def NearestPoints(self, points, signed=False, winding_beta=None):
        """tb_nearest_points: for every point the nearest point of the scene's triangles (include/tb_nearest.h has the rule).  A numpy array --
        QUERY_POINT_DTYPE (make_query_points), or float32 of shape (n, 4): position, MaxDistance -- takes the host path and returns a NEAREST_DTYPE
        array.  A torch tensor, float32 (n, 4), contiguous, 16-B aligned, on the context's device, takes the device path with zero copy: torch's
        current stream on that device is synchronised first, and the result is a float32 (n, 8) tensor -- Point, Distance, U, V, then Prim and Geom
        through .view(torch.int32).  signed: Distance is negative behind the nearest triangle.  winding_beta, a number >= 1
        (tb_nearest_points_winding): Distance is negative where the winding number says inside, the robust sign; not together
        with signed.  Anything else: ValueError, before any library call."""
        on_device = _check_query_points("NearestPoints", points, getattr(self, "_device", 0))
        flags = NEAREST_SIGNED if _check_flag("NearestPoints", "signed", signed) else 0
        beta = None if winding_beta is None else _check_beta("NearestPoints", winding_beta, "winding_beta")
        if beta is not None and signed:
            raise ValueError("NearestPoints: signed and winding_beta are two rules for the sign: give one")
        n = int(points.shape[0])

        def call(dev, ptr, o):
            if beta is None:
                return self._L.tb_nearest_points(self._ctx, flags | dev, n, ptr(points), o)
            return self._L.tb_nearest_points_winding(self._ctx, flags | dev, n, ptr(points), beta, o)
        return self._query(on_device, NEAREST_DEVICE, call, (n, 8), n, NEAREST_DTYPE)

    def BakeDistanceField(self, grid, signed=False, max_distance=np.inf, device=False, winding_beta=None):
        """tb_bake_distance_field: float32 of shape (count[2], count[1], count[0]) -- for every cell of the ProbeGrid the Distance of NearestPoints at
        origin + (i, j, k) * spacing with MaxDistance = max_distance (+inf where nothing is that near); the positions are made in the kernel.
        device=True: a torch tensor on the context's device that torch allocated, zero copy; else a numpy array.  winding_beta: as NearestPoints'
        (tb_bake_distance_field_winding)."""
        _check_distance_field(grid, signed, max_distance, device)
        beta = None if winding_beta is None else _check_beta("BakeDistanceField", winding_beta, "winding_beta")
        if beta is not None and signed:
            raise ValueError("BakeDistanceField: signed and winding_beta are two rules for the sign: give one")
        flags = NEAREST_SIGNED if signed else 0
        g = grid.c_struct()
        shape = (grid.count[2], grid.count[1], grid.count[0])

        def call(dev, ptr, o):
            if beta is None:
                return self._L.tb_bake_distance_field(self._ctx, flags | dev, C.byref(g), float(max_distance), o)
            return self._L.tb_bake_distance_field_winding(self._ctx, flags | dev, C.byref(g), float(max_distance), beta, o)
        return self._query(device, NEAREST_DEVICE, call, shape, shape)

    # -- winding numbers ----------------------------------------------------
    def WindingNumbers(self, points, beta=WINDING_BETA, host_walk=False):
        """tb_winding_numbers: for every point the generalized winding number of the scene's triangles (include/tb_winding.h has the rule; 1 inside
        a closed outward-facing mesh, 0 outside; api.winding_inside(w) is the test).  points as NearestPoints' -- MaxDistance is not read: a numpy
        array takes the host path and returns float32 (n,); a torch tensor on the context's device the device path with zero copy, and returns a
        float32 (n,) tensor.  beta >= 1: a subtree farther than beta radii is one dipole; inf sums every triangle.  host_walk=True (numpy only): the
        same walk as scalar C++ over the context's host copies of the tree, which the device equals on bits."""
        on_device = _check_query_points("WindingNumbers", points, getattr(self, "_device", 0))
        beta = _check_beta("WindingNumbers", beta)
        if _check_flag("WindingNumbers", "host_walk", host_walk) and on_device:
            raise ValueError("WindingNumbers: host_walk takes a numpy array")
        n = int(points.shape[0])
        flags = WINDING_HOST_WALK if host_walk else 0

        def call(dev, ptr, o):
            return self._L.tb_winding_numbers(self._ctx, flags | dev, n, ptr(points), beta, o)
        return self._query(on_device, WINDING_DEVICE, call, (n,), n)

    def BakeWindingField(self, grid, beta=WINDING_BETA, device=False):
        """tb_bake_winding_field: float32 of shape (count[2], count[1], count[0]) -- for every cell of the ProbeGrid the WindingNumbers at
        origin + (i, j, k) * spacing; the positions are made in the kernel.  device=True: a torch tensor on the context's device, zero copy."""
        if not isinstance(grid, ProbeGrid):
            raise ValueError("BakeWindingField: grid is a ProbeGrid, not %s" % type(grid).__name__)
        beta = _check_beta("BakeWindingField", beta)
        _check_flag("BakeWindingField", "device", device)
        if grid.n > 1 << 31:
            raise ValueError("BakeWindingField: more than 2^31 cells")
        g = grid.c_struct()
        shape = (grid.count[2], grid.count[1], grid.count[0])

        def call(dev, ptr, o):
            return self._L.tb_bake_winding_field(self._ctx, dev, C.byref(g), beta, o)
        return self._query(device, WINDING_DEVICE, call, shape, shape)

    # -- radiance queries ---------------------------------------------------
    def TraceRadiance(self, rays, samples=1, first_sample=0, seed_advance=0.0, mode=RADIANCE_RAY, settings=None, time=0.0, out=None):
        """tb_trace_radiance: the path tracer on the caller's rays; per ray (sum r, sum g, sum b, accepted samples) of the samples
        [first_sample, first_sample + samples), summed in sample order.  mode RADIANCE_HEMISPHERE: the directions are unit normals and every sample
        starts along a cosine-weighted direction about it (pi * sum / count is the irradiance).  A numpy array -- RADIANCE_RAY_DTYPE
        (make_radiance_rays), or float32 (n, 8) -- takes the host path and returns a float32 (n, 4) array; a torch tensor, float32 (n, 8), contiguous,
        16-B aligned, on the context's device, takes the device path with zero copy after torch's current stream on that device is synchronised, and
        returns a tensor.  out given (float32 (n, 4), of the rays' kind): the sums start from it, and it is returned.  Anything else: ValueError,
        before any library call."""
        on_device = _check_radiance_call(rays, samples, first_sample, seed_advance, mode, out, getattr(self, "_device", 0))
        n = int(rays.shape[0])
        flags = mode | (RADIANCE_ACCUMULATE if out is not None else 0)

        def call(dev, ptr, o):
            k = abi.TbRadianceCall(int(first_sample), int(samples), float(seed_advance), flags | dev)
            return self._L.tb_trace_radiance(self._ctx, _ref(settings), time, C.byref(k), n, ptr(rays), o)
        return self._query(on_device, RADIANCE_DEVICE, call, (n, 4), (n, 4), out=out)

    def MakeCameraRays(self, width, height, frame, window=None, settings=None, time=0.0, device=False):
        """tb_make_camera_rays: (rays, seed_advance) -- the renderer's camera rays of frame `frame` for the pixels of window = (x0, y0, x1, y1)
        (half-open; default the whole width x height picture), row-major in the window, and how far path_begin moved the seed: TraceRadiance(rays, 1,
        frame, seed_advance) adds what Render adds to the accumulation in that frame.  rays: a RADIANCE_RAY_DTYPE array, or (device) a float32
        (n, 8) tensor on the context's device."""
        for name, v in (("width", width), ("height", height)):
            _check_count("MakeCameraRays", name, v, 1, 16384)
        _check_count("MakeCameraRays", "frame", frame, 0, 0xffffffff)
        x0, y0, x1, y1 = (0, 0, width, height) if window is None else window
        for name, v in (("x0", x0), ("y0", y0), ("x1", x1), ("y1", y1)):
            _check_count("MakeCameraRays", name, v, 0, 16384)
        if not (x0 < x1 <= width and y0 < y1 <= height):
            raise ValueError("MakeCameraRays: the window (%d, %d, %d, %d) is empty or leaves the %d x %d picture" % (x0, y0, x1, y1, width, height))
        n = (x1 - x0) * (y1 - y0)
        advance = C.c_float(0.0)

        def call(dev, ptr, o):
            return self._L.tb_make_camera_rays(self._ctx, _ref(settings), time, width, height, x0, y0, x1, y1, frame, dev, o, C.byref(advance))
        rays = self._query(device, RADIANCE_DEVICE, call, (n, 8), n, RADIANCE_RAY_DTYPE)
        return rays, advance.value

    # -- lightmap baking ---------------------------------------------------
    def BakeLightmap(self, width, height, samples, uv=None, first_sample=0, dilate=2, accumulate=False, settings=None, time=0.0, out=None):
        """tb_bake_lightmap: the scene's triangles rasterised into a width x height atlas by their lightmap UVs, every owned texel traced over the
        samples [first_sample, first_sample + samples) of its cosine-weighted hemisphere, the sums resolved to irradiance (alpha 1) and the gutters
        filled by `dilate` 3 x 3 passes (alpha 2^-pass).  Returns the (height, width, 4) float32 picture, row 0 = v 0.  uv: (numVertices, 2) float32,
        one pair per vertex of the scene; None: the UV field of the scene's vertex records (loads flip V).  accumulate: add the samples to the last
        bake of this size instead of rasterising again.  uv and out may be numpy arrays (the host path) or contiguous torch tensors on the
        context's device (zero copy, after torch's current stream there is synchronised; the picture is then a tensor).  Anything else:
        ValueError, before any library call."""
        on_device = _check_bake_call(width, height, samples, uv, first_sample, dilate, accumulate, out, getattr(self, "_device", 0))
        if uv is not None and not accumulate:
            info = abi.tb_scene_info()
            if self._L.tb_scene_info_get(self._ctx, C.byref(info)) == 0 and int(uv.shape[0]) != info.numVertices:
                raise ValueError("BakeLightmap: uv has %d pairs, the scene %d vertices" % (int(uv.shape[0]), info.numVertices))
        def call(dev, ptr, o):
            k = abi.tb_bake_call(int(width), int(height), int(first_sample), int(samples), int(dilate), (BAKE_ACCUMULATE if accumulate else 0) | dev)
            return self._L.tb_bake_lightmap(self._ctx, _ref(settings), time, C.byref(k), ptr(uv) if uv is not None else None, o)
        shape = (height, width, 4)
        return self._query(on_device, BAKE_DEVICE, call, shape, shape, out=out)

    def ReadBake(self):
        """tb_read_bake: (rays, texels, sums) of the last bake -- RADIANCE_RAY_DTYPE and BAKE_TEXEL_DTYPE arrays of shape (height, width) and the
        float32 (height, width, 4) sums (sum r, sum g, sum b, accepted samples) the picture was resolved from."""
        w, h = int(self._L.tb_get_option(self._ctx, b"bake_width")), int(self._L.tb_get_option(self._ctx, b"bake_height"))
        if not w or not h:
            self._check(self._L.tb_read_bake(self._ctx, None, None, None))   # the library's own refusal: no bake is held
        rays = np.empty((h, w), RADIANCE_RAY_DTYPE); texels = np.empty((h, w), BAKE_TEXEL_DTYPE); sums = np.empty((h, w, 4), np.float32)
        self._check(self._L.tb_read_bake(self._ctx, _np_ptr(rays), _np_ptr(texels), _np_ptr(sums)))
        return rays, texels, sums

    def RunBakeRaster(self, width, height, positions, normals, uvs, tri_vertex_index):
        """bake_cover + bake_texels on host arrays, no scene: positions, normals (n, 3) and uvs (n, 2) float32, tri_vertex_index (t, 3) uint32.
        Returns (rays, texels): RADIANCE_RAY_DTYPE and BAKE_TEXEL_DTYPE arrays of shape (height, width)."""
        _check_count("RunBakeRaster", "width", width, 1, BAKE_MAX_SIDE)
        _check_count("RunBakeRaster", "height", height, 1, BAKE_MAX_SIDE)
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uvs, np.float32).reshape(-1, 2); tri = np.ascontiguousarray(tri_vertex_index, np.uint32).reshape(-1, 3)
        if nrm.shape[0] != p.shape[0] or uv.shape[0] != p.shape[0]:
            raise ValueError("RunBakeRaster: positions, normals and uvs have one entry per vertex")
        if tri.size and int(tri.max()) >= p.shape[0]:
            raise ValueError("RunBakeRaster: a vertex number is not below the number of vertices")
        rays = np.empty((height, width), RADIANCE_RAY_DTYPE); texels = np.empty((height, width), BAKE_TEXEL_DTYPE)
        self._check(self._L.tb_run_bake_raster(self._ctx, width, height, p.shape[0], _np_ptr(p), _np_ptr(nrm), _np_ptr(uv), tri.shape[0], _np_ptr(tri),
                                               _np_ptr(rays), _np_ptr(texels)))
        return rays, texels

    def RunBakeDilate(self, rgba, passes):
        """bake_dilate on a host picture: `passes` 3 x 3 fill passes of an (H, W, 4) float32 array; returns the filled picture."""
        a = np.ascontiguousarray(rgba, np.float32)
        if a.ndim != 3 or a.shape[2] != 4 or not a.shape[0] or not a.shape[1] or a.shape[0] > BAKE_MAX_SIDE or a.shape[1] > BAKE_MAX_SIDE:
            raise ValueError("RunBakeDilate: rgba is an (H, W, 4) picture with sides of 1 to %d" % BAKE_MAX_SIDE)
        _check_count("RunBakeDilate", "passes", passes, 0, BAKE_MAX_DILATE)
        out = np.empty_like(a)
        self._check(self._L.tb_run_bake_dilate(self._ctx, a.shape[1], a.shape[0], passes, _np_ptr(a), _np_ptr(out)))
        return out

    # -- light probes -------------------------------------------------------
    def BakeProbes(self, positions, resolution=16, samples=64, first_sample=0, first_number=0, keep_maps=False, accumulate=False, settings=None, time=0.0):
        """tb_bake_probes: one SH9 probe per position -- the radiance along the resolution x resolution directions of an octahedral map, `samples`
        paths each (the samples [first_sample, first_sample + samples)), projected onto nine SH basis functions, and the hit statistics of the same
        directions.  positions: float32 (n, 3), a numpy array (returns a PROBE_DTYPE array (n,)) or a contiguous torch tensor on the context's
        device (zero copy, after torch's current stream there is synchronised; returns a float32 (n, 32) tensor).  first_number: the number of the
        first probe, which seeds its paths -- a probe keeps its record wherever it stands in a call.  keep_maps: the context keeps every ray's sums and
        hits (ReadProbeMaps); accumulate: add the samples to the bake kept.  Anything else: ValueError, before any library call."""
        on_device = _check_probe_call(positions, resolution, samples, first_sample, first_number, keep_maps, accumulate, getattr(self, "_device", 0))
        n = int(positions.shape[0])
        flags = (PROBES_KEEP_MAPS if keep_maps else 0) | (PROBES_ACCUMULATE if accumulate else 0)

        def call(dev, ptr, o):
            k = abi.tb_probe_call(n, int(first_number), int(resolution), int(first_sample), int(samples), flags | dev)
            return self._L.tb_bake_probes(self._ctx, _ref(settings), time, C.byref(k), ptr(positions), o)
        return self._query(on_device, PROBES_DEVICE, call, (n, 32), n, PROBE_DTYPE)

    def ReadProbeMaps(self):
        """tb_read_probe_maps: (sums, hits) of the last bake that kept its maps -- float32 (n, M * M, 4) (sum r, sum g, sum b, accepted samples) and
        QUERY_HIT_DTYPE (n, M * M), ray t = y * M + x of probe i at [i, t]."""
        n, m = int(self._L.tb_get_option(self._ctx, b"probes_held")), int(self._L.tb_get_option(self._ctx, b"probes_resolution"))
        if not n or not int(self._L.tb_get_option(self._ctx, b"probes_maps_held")):
            self._check(self._L.tb_read_probe_maps(self._ctx, None, None))   # the library's own refusal: no maps are held
        sums = np.empty((n, m * m, 4), np.float32); hits = np.empty((n, m * m), QUERY_HIT_DTYPE)
        self._check(self._L.tb_read_probe_maps(self._ctx, _np_ptr(sums), _np_ptr(hits)))
        return sums, hits

    def SampleProbes(self, grid, probes, points, normals, resolution=16, backface_limit=0.25):
        """tb_sample_probes: float (n, 4) -- the irradiance (r, g, b) of a probe grid at the points with the unit normals, and the sum of the
        trilinear weights of the probes that counted (0: none was near, the irradiance is zeros).  grid: a ProbeGrid; probes: its records as
        BakeProbes returned them (resolution: that bake's); a probe counts iff its Weight > 0 and its Backfaces <= backface_limit * resolution^2
        (0.25 is DDGI's convention).  numpy arrays all, or torch tensors on the context's device all.  Anything else: ValueError, before any
        library call."""
        if not isinstance(grid, ProbeGrid):
            raise ValueError("SampleProbes: grid is a ProbeGrid")
        _check_count("SampleProbes", "resolution", resolution, PROBE_MIN_RES, PROBE_MAX_RES)
        if isinstance(backface_limit, bool) or not isinstance(backface_limit, (int, float, np.integer, np.floating)) or np.isnan(backface_limit):
            raise ValueError("SampleProbes: backface_limit is a number, not %r" % (backface_limit,))
        device = getattr(self, "_device", 0)
        on_device = _check_array("SampleProbes", "probes", probes, device, columns=32, record_dtype=PROBE_DTYPE, align=16, rows=grid.n)
        if _check_array("SampleProbes", "points", points, device, columns=3) != on_device or \
                _check_array("SampleProbes", "normals", normals, device, columns=3, rows=int(points.shape[0])) != on_device:
            raise ValueError("SampleProbes: probes, points and normals are numpy arrays all, or torch tensors all")
        n = int(points.shape[0])
        g = grid.c_struct()

        def call(dev, ptr, o):
            return self._L.tb_sample_probes(self._ctx, dev, C.byref(g), resolution, float(backface_limit), ptr(probes), n, ptr(points), ptr(normals), o)
        return self._query(on_device, PROBES_DEVICE, call, (n, 4), (n, 4))

    def RunProbeRays(self, positions, resolution, first_number=0):
        """probe_rays on host positions (n, 3), no scene: (RADIANCE_RAY_DTYPE, QUERY_RAY_DTYPE) arrays of shape (n, M * M)."""
        _check_count("RunProbeRays", "resolution", resolution, PROBE_MIN_RES, PROBE_MAX_RES)
        p = np.ascontiguousarray(positions, np.float32)
        if p.ndim != 2 or p.shape[1] != 3 or not p.shape[0] or p.shape[0] * resolution * resolution > 1 << 24:
            raise ValueError("RunProbeRays: positions are (n, 3), 1 <= n, at most 2^24 rays")
        _check_count("RunProbeRays", "first_number", first_number, 0, PROBE_MAX_PROBES - p.shape[0])
        rad = np.empty((p.shape[0], resolution * resolution), RADIANCE_RAY_DTYPE); qry = np.empty(rad.shape, QUERY_RAY_DTYPE)
        self._check(self._L.tb_run_probe_rays(self._ctx, p.shape[0], resolution, first_number, _np_ptr(p), _np_ptr(rad), _np_ptr(qry)))
        return rad, qry

    def RunProbeProject(self, positions, resolution, sums, hits):
        """probe_project on host arrays, no scene: positions (n, 3), sums float32 (n, M * M, 4), hits QUERY_HIT_DTYPE (n, M * M); PROBE_DTYPE (n,)."""
        _check_count("RunProbeProject", "resolution", resolution, PROBE_MIN_RES, PROBE_MAX_RES)
        p = np.ascontiguousarray(positions, np.float32)
        if p.ndim != 2 or p.shape[1] != 3 or not p.shape[0] or p.shape[0] * resolution * resolution > 1 << 24:
            raise ValueError("RunProbeProject: positions are (n, 3), 1 <= n, at most 2^24 rays")
        sm = np.ascontiguousarray(sums, np.float32); ht = np.ascontiguousarray(hits)
        if sm.shape != (p.shape[0], resolution * resolution, 4) or ht.dtype != QUERY_HIT_DTYPE or ht.shape != sm.shape[:2]:
            raise ValueError("RunProbeProject: sums are float32 (n, M * M, 4) and hits QUERY_HIT_DTYPE (n, M * M)")
        out = np.empty(p.shape[0], PROBE_DTYPE)
        self._check(self._L.tb_run_probe_project(self._ctx, p.shape[0], resolution, _np_ptr(p), _np_ptr(sm), _np_ptr(ht), _np_ptr(out)))
        return out

    # -- dynamic scenes ----------------------------------------------------
    def _update_vertices(self, what, fn_name, a, first):
        on_device = _check_vertex_array(what, a, first, getattr(self, "_device", 0))
        n = int(a.shape[0])
        fn = getattr(self._L, fn_name)
        if on_device:
            _torch_sync(a.device)
            self._check(fn(self._ctx, UPDATE_DEVICE, first, n, C.c_void_p(a.data_ptr() or None)))
            self._check(self._L.tb_sync(self._ctx))                 # the tensor has been read: torch may give its memory to another
        else:
            self._check(fn(self._ctx, 0, first, n, _np_ptr(a)))

    def UpdatePositions(self, a, first=0):
        """tb_update_positions: stage new positions of the vertices first .. first + n.  a: float32 (n, 3), a numpy array (checked for finite values)
        or a contiguous torch tensor on the context's device (read where it lies, values unchecked).  Anything else: ValueError, before any library
        call.  Nothing changes until CommitGeometry."""
        self._update_vertices("UpdatePositions", "tb_update_positions", a, first)

    def UpdateNormals(self, a, first=0):
        """tb_update_normals: stage new shading normals (the Normal field of the vertex records) of the vertices first .. first + n; a as for UpdatePositions."""
        self._update_vertices("UpdateNormals", "tb_update_normals", a, first)

    def RecomputeNormals(self, first=0, n=None):
        """tb_recompute_normals: mark the vertices first .. first + n (None: to the end); the next CommitGeometry makes their smooth normals again on
        the device from the positions it leaves (include/tb_normals.h).  Vertices of emissive geometries are skipped."""
        for name, v in (("first", first), ("n", 0 if n is None else n)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > 0xffffffff:
                raise ValueError("RecomputeNormals: %s is a vertex count, not %r" % (name, v))
        if n is None:
            if getattr(self, "_num_vertices", None) is None:       # asked once per load: the question brings stale host copies up
                self._num_vertices = int(self.SceneInfo().numVertices)
            n = max(self._num_vertices - first, 0)
        self._check(self._L.tb_recompute_normals(self._ctx, first, n))

    def SetInstanceTransforms(self, m, first=0):
        """tb_set_instance_transforms: stage objectToWorld of the instances first .. first + n of a two-level scene; m: float32 (n, 3, 4) or (n, 12)."""
        if isinstance(first, bool) or not isinstance(first, (int, np.integer)) or first < 0 or first > 0xffffffff:
            raise ValueError("SetInstanceTransforms: first is an instance number, not %r" % (first,))
        if not isinstance(m, np.ndarray) or m.dtype != np.float32 or not (m.ndim == 3 and m.shape[1:] == (3, 4) or m.ndim == 2 and m.shape[1] == 12):
            raise ValueError("SetInstanceTransforms: m is a float32 numpy array of shape (n, 3, 4) or (n, 12)")
        if not m.flags["C_CONTIGUOUS"]:
            raise ValueError("SetInstanceTransforms: the array is not contiguous")
        self._check(self._L.tb_set_instance_transforms(self._ctx, first, int(m.shape[0]), _np_ptr(m)))

    def CommitGeometry(self, rebuild=False):
        """tb_commit_geometry: apply what was staged -- a refit of the tree as it stands, or (rebuild) the tree a fresh load of the moved scene builds."""
        self._check(self._L.tb_commit_geometry(self._ctx, GEOMETRY_REBUILD if rebuild else 0))

    def GeometryVertexRange(self, g):
        """tb_geometry_vertex_range: (first vertex, number of vertices) of geometry (hit-group record) g."""
        first, count = C.c_uint32(), C.c_uint32()
        self._check(self._L.tb_geometry_vertex_range(self._ctx, int(g), C.byref(first), C.byref(count)))
        return first.value, count.value

    def DeviceMath(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        b2 = np.ascontiguousarray(b, np.float32) if b is not None else None
        out = np.empty_like(a)
        self._check(self._L.tb_device_math(self._ctx, fn, a.size, _np_ptr(a), _np_ptr(b2) if b2 is not None else None, _np_ptr(out)))
        return out

    # the real-time kernels on host surfaces (tb_run_*): (H, W, 4) float32 arrays, no scene, nothing of the context read or written
    def RunTemporal(self, constants, history, current, world_pos, prev_world_pos, moment_history, normals):
        """rt_temporal_kernel; returns (out, moments), moments None unless constants.OutputMomentInformation."""
        f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (history, current, world_pos, prev_world_pos, moment_history, normals)]
        shape = (constants.ResolutionY, constants.ResolutionX, 4)
        out = np.empty(shape, np.float32)
        mom = np.empty(shape, np.float32) if constants.OutputMomentInformation and moment_history is not None else None
        self._check(self._L.tb_run_temporal(self._ctx, C.byref(constants), *[None if a is None else _np_ptr(a) for a in f], _np_ptr(out),
                                            None if mom is None else _np_ptr(mom)))
        return out, mom

    def RunDenoisePass(self, constants, inp, normals, positions, undenoised):
        """rt_denoise_kernel: one a-trous pass."""
        f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (inp, normals, positions, undenoised)]
        out = np.empty((constants.ResolutionY, constants.ResolutionX, 4), np.float32)
        self._check(self._L.tb_run_denoise_pass(self._ctx, C.byref(constants), *[None if a is None else _np_ptr(a) for a in f], _np_ptr(out)))
        return out

    def RunComposite(self, width, height, albedo, lighting, emissive):
        """rt_composite_kernel."""
        f = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (albedo, lighting, emissive)]
        out = np.empty((height, width, 4), np.float32)
        self._check(self._L.tb_run_composite(self._ctx, width, height, *[None if a is None else _np_ptr(a) for a in f], _np_ptr(out)))
        return out

    # -- sample budgets ---------------------------------------------------
    def SetSampleBudget(self, budget):
        """budget: an (H, W) uint32 array -- per pixel the global frame index at which it stops receiving samples -- or None to clear it
        (tb_set_sample_budget).  While one is set a Render that starts at frame F0 gives pixel p all of its frames iff F0 < budget[p]."""
        if budget is None:
            self._check(self._L.tb_set_sample_budget(self._ctx, 0, 0, None))
            self._budget_shape = None
            return
        b = np.ascontiguousarray(budget, np.uint32)
        if b.ndim != 2:
            raise ValueError("SetSampleBudget: an (H, W) array")
        self._check(self._L.tb_set_sample_budget(self._ctx, b.shape[1], b.shape[0], _np_ptr(b)))
        self._budget_shape = b.shape

    def SampleBudget(self):
        """The budget the context holds, (H, W) uint32 (tb_read_sample_budget); TracerBoyError without one."""
        out = np.empty(self._budget_shape or (max(self.height, 1), max(self.width, 1)), np.uint32)
        self._check(self._L.tb_read_sample_budget(self._ctx, _np_ptr(out)))
        return out

    def StopConverged(self, rel_error, min_frames=64):
        """The noise target (tb_budget_stop_converged): every live pixel whose estimated relative error is below rel_error stops at the current
        frame.  Returns (pixels stopped by this call, pixels still live)."""
        stopped, live = C.c_uint64(), C.c_uint64()
        self._check(self._L.tb_budget_stop_converged(self._ctx, rel_error, min_frames, C.byref(stopped), C.byref(live)))
        self._budget_shape = self._budget_shape or (self.height, self.width)     # (the call makes an all-live budget where there is none)
        return int(stopped.value), int(live.value)

    def RunBudgetStop(self, output, jittered, budget, rel_error, min_frames, frame):
        """budget_stop_kernel behind section 12's prepare and prefilter, on host arrays (tb_run_budget_stop): (H, W, 4) float32 sums, (H, W) uint32
        budget.  Returns (the budget afterwards, stopped, live)."""
        o, q = np.ascontiguousarray(output, np.float32), np.ascontiguousarray(jittered, np.float32)
        b = np.array(budget, np.uint32, order="C")
        stopped, live = C.c_uint64(), C.c_uint64()
        self._check(self._L.tb_run_budget_stop(self._ctx, o.shape[1], o.shape[0], _np_ptr(o), _np_ptr(q), _np_ptr(b), rel_error, min_frames, frame,
                                               C.byref(stopped), C.byref(live)))
        return b, int(stopped.value), int(live.value)


def unpack_gathered(width, height, world, tile_w, tile_h, per_rank_packed):
    """Rank-0 un-permute of gathered per-rank tile buffers (tb_unpack_gathered_host)."""
    arrs = [np.ascontiguousarray(a, np.float32) for a in per_rank_packed]
    ptrs = (C.c_void_p * world)(*[a.ctypes.data for a in arrs])
    full = np.zeros((height, width, 4), np.float32)
    rc = lib().tb_unpack_gathered_host(width, height, world, tile_w, tile_h, ptrs, _np_ptr(full))
    if rc != 0:
        raise TracerBoyError(rc, "tb_unpack_gathered_host")
    return full
