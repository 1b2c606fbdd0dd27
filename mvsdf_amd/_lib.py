"""ctypes binding of libmvsdf_hip.so (C ABI: include/mvsdf_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, we raise.
"""
import ctypes as C
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get('MVSDF_LIB') or os.path.join(_HERE, 'libmvsdf_hip.so')   # MVSDF_LIB: dev override (ablation builds)
MAX_LAYERS = 12
_lib = None


class NetDesc(C.Structure):
    _fields_ = [('n_layers', C.c_int), ('K', C.c_int * MAX_LAYERS), ('N', C.c_int * MAX_LAYERS),
                ('wp', C.c_void_p * MAX_LAYERS), ('bias', C.c_void_p * MAX_LAYERS), ('w', C.c_void_p * MAX_LAYERS),
                ('skip_layer', C.c_int), ('multires', C.c_int), ('wp16', C.c_void_p * MAX_LAYERS), ('trace_dtype', C.c_int), ('skip_mask', C.c_uint), ('wx3', C.c_void_p * MAX_LAYERS)]


class TraceParams(C.Structure):
    _fields_ = [('r', C.c_float), ('thr', C.c_float), ('line_search_step', C.c_float), ('line_step_iters', C.c_int),
                ('st_iters', C.c_int), ('n_steps', C.c_int), ('n_secant', C.c_int), ('dist_clip', C.c_float)]


class MvsdfError(RuntimeError):
    pass


def lib():
    """Load the HIP library (built in-tree by mvsdf_amd/build.py).  Raises if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise MvsdfError('libmvsdf_hip.so not found at %s -- run `python -c "import __graft_entry__ as g; g.build()"` '
                             '(hipcc --offload-arch=gfx950); there is no CPU/PyTorch fallback for the hot path' % SO_PATH)
        import torch  # noqa: F401  -- load torch's bundled HIP runtime first so this library binds to the same libamdhip64
        L = C.CDLL(SO_PATH)
        L.mvsdf_last_error.restype = C.c_char_p
        L.mvsdf_packed_floats.restype = C.c_size_t
        L.mvsdf_packed_floats.argtypes = [C.c_int, C.c_int]
        L.mvsdf_trace_workspace_bytes.restype = C.c_size_t
        L.mvsdf_trace_workspace_bytes.argtypes = [C.c_int]
        L.mvsdf_trace_workspace_bytes_n.restype = C.c_size_t
        L.mvsdf_trace_workspace_bytes_n.argtypes = [C.c_int, C.c_int]
        L.mvsdf_trace_cut_workspace_bytes.restype = C.c_size_t
        L.mvsdf_trace_cut_workspace_bytes.argtypes = [C.c_int, C.c_int]
        for fn in ('mvsdf_sdf_ctx_floats', 'mvsdf_sdf_bwd_ws_floats', 'mvsdf_render_ctx_floats', 'mvsdf_render_bwd_ws_floats'):
            getattr(L, fn).restype = C.c_size_t
        L.mvsdf_adam_ws_floats.restype = C.c_size_t
        L.mvsdf_packed_bf16_bytes.restype = C.c_size_t
        L.mvsdf_packed_bf16_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.mvsdf_tracegen_state_bytes.restype = C.c_size_t
        L.mvsdf_adam_step.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_float, C.c_double, C.c_double, C.c_float] + [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mvsdf_adam_step_scaled.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_float, C.c_double, C.c_double, C.c_float] + [C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mvsdf_adam_step_fused.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_float, C.c_double, C.c_double, C.c_float] + [C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mvsdf_loss_scale.argtypes = [C.c_void_p] + [C.c_float] * 5 + [C.c_void_p, C.c_void_p, C.c_int] * 4 + [C.c_void_p, C.c_void_p]   # g: host array of 6 pointers
        i64, vp, f32 = C.c_int64, C.c_void_p, C.c_float
        L.mvsdf_mc_workspace_bytes.restype = C.c_size_t
        L.mvsdf_mc_workspace_bytes.argtypes = [i64] * 3
        L.mvsdf_mc_count.argtypes = [vp, vp, vp, f32, vp, C.c_size_t, vp]
        L.mvsdf_mc_emit.argtypes = [vp, vp, vp, f32, vp, vp, vp, C.c_size_t, vp, vp, vp, i64, i64, vp]
        L.mvsdf_mesh_cc_workspace_bytes.restype = C.c_size_t
        L.mvsdf_mesh_cc_workspace_bytes.argtypes = [i64, i64]
        L.mvsdf_mesh_components.argtypes = [vp, vp, i64, i64, vp, C.c_size_t, vp, vp, vp]
        L.mvsdf_mesh_select.argtypes = [vp, vp, i64, i64, C.c_int32] + [vp] * 5 + [C.c_size_t] + [vp] * 4 + [i64, i64, vp]
        L.mvsdf_smc_workspace_bytes.restype = C.c_size_t
        L.mvsdf_smc_workspace_bytes.argtypes = [i64, i64]
        L.mvsdf_smc_emit_workspace_bytes.restype = C.c_size_t
        L.mvsdf_smc_emit_workspace_bytes.argtypes = [i64, i64, i64]
        L.mvsdf_smc_coarse_points.argtypes = [vp, i64, i64, i64, i64, vp, vp]
        L.mvsdf_smc_seed.argtypes = [vp, i64, i64, f32, f32, vp, C.c_size_t, vp]
        L.mvsdf_smc_brick_points.argtypes = [vp, i64, i64, vp, C.c_size_t, i64, i64, vp, vp]
        L.mvsdf_smc_closure.argtypes = [vp, i64, i64, f32, i64, i64, vp, C.c_size_t, vp]
        L.mvsdf_smc_count.argtypes = [vp, i64, i64, f32, i64, vp, C.c_size_t, vp, C.c_size_t, vp]
        L.mvsdf_smc_emit.argtypes = [vp, i64, i64, f32, vp, vp, i64, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, i64, i64, vp]
        L.mvsdf_mesh_cut_workspace_bytes.restype = C.c_size_t
        L.mvsdf_mesh_cut_workspace_bytes.argtypes = [i64, i64]
        L.mvsdf_mesh_cut.argtypes = [vp, vp, i64, i64, C.c_int32, C.c_int32, vp, C.c_size_t, vp, vp]
        L.mvsdf_mesh_trim.argtypes = [vp] * 4 + [i64, i64, vp, C.c_size_t] + [vp] * 4 + [i64, i64, vp]
        f64, u64, sz = C.c_double, C.c_uint64, C.c_size_t
        L.mvsdf_mesh_simplify_workspace_bytes.restype = sz
        L.mvsdf_mesh_simplify_workspace_bytes.argtypes = [i64, i64]
        L.mvsdf_mesh_simplify.argtypes = [vp] * 4 + [i64, i64, f64, vp, C.c_int32, C.c_int32, vp, sz, vp]
        L.mvsdf_mesh_simplify_emit.argtypes = [vp, i64, i64, vp, sz] + [vp] * 4 + [i64, i64, vp]
        L.mvsdf_chamfer_key.restype = u64
        L.mvsdf_chamfer_key.argtypes = [u64, i64]
        for fn in ('mvsdf_chamfer_sample_workspace_bytes', 'mvsdf_chamfer_mask_workspace_bytes', 'mvsdf_chamfer_nearest_workspace_bytes'):
            getattr(L, fn).restype = sz
            getattr(L, fn).argtypes = [i64, i64]
        L.mvsdf_chamfer_downsample_workspace_bytes.restype = sz
        L.mvsdf_chamfer_downsample_workspace_bytes.argtypes = [i64]
        L.mvsdf_chamfer_sample_count.argtypes = [vp, vp, i64, i64, f64, i64, vp, sz, vp]
        L.mvsdf_chamfer_sample_emit.argtypes = [vp, vp, i64, i64, f64, vp, sz, vp, i64, vp]
        L.mvsdf_chamfer_downsample.argtypes = [vp, i64, f64, u64, i64, vp, sz, vp, vp]
        L.mvsdf_chamfer_mask.argtypes = [vp, vp, i64, vp, i64, vp, f64, vp, vp, vp, vp, sz, vp, vp, vp, vp]
        L.mvsdf_chamfer_nearest.argtypes = [vp, i64, vp, i64, f64, vp, sz, vp, vp]
        i32 = C.c_int32
        L.mvsdf_fusion_workspace_bytes.restype = sz
        L.mvsdf_fusion_workspace_bytes.argtypes = [i64] * 4
        L.mvsdf_fusion_fuse.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, f64, f64, vp, sz, vp, vp, vp, vp]
        L.mvsdf_fusion_emit.argtypes = [vp, i64, i64, i64, i64, vp, sz, vp, vp, vp, vp, i64, vp]
        L.mvsdf_fusion_normals_workspace_bytes.restype = sz
        L.mvsdf_fusion_normals_workspace_bytes.argtypes = [i64]
        L.mvsdf_fusion_normals.argtypes = [vp, i64, i64, i64, vp, vp, i64, vp, f64, vp, sz, vp, vp]
        L.mvsdf_poisson_workspace_bytes.restype = sz
        L.mvsdf_poisson_workspace_bytes.argtypes = [i64, i32]
        L.mvsdf_poisson_reconstruct.argtypes = [vp, vp, i64, vp, f64, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp]
        L.mvsdf_poisson_valid.argtypes = [vp, i32, f64, i32, vp, vp, vp]
        L.mvsdf_poisson_volume.argtypes = [vp, i64, f64, vp, vp]
        L.mvsdf_tsdf_workspace_bytes.restype = sz
        L.mvsdf_tsdf_workspace_bytes.argtypes = [i64] * 4
        L.mvsdf_tsdf_integrate.argtypes = [vp, i64, i64, i64, vp, vp, i64, vp, f64, vp, f64, f64, i32, vp, sz, vp, vp, vp, vp]
        L.mvsdf_mcm_workspace_bytes.restype = sz
        L.mvsdf_mcm_workspace_bytes.argtypes = [i64] * 3
        L.mvsdf_mcm_count.argtypes = [vp, vp, vp, vp, f32, vp, sz, vp]
        L.mvsdf_mcm_emit.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp, sz, vp, vp, vp, i64, i64, vp]
        for fn in ('mvsdf_cloud_clean_workspace_bytes', 'mvsdf_cloud_compact_workspace_bytes'):
            getattr(L, fn).restype = sz
            getattr(L, fn).argtypes = [i64]
        L.mvsdf_cloud_knn.argtypes = [vp, i64, i32, vp, sz, vp, vp]
        L.mvsdf_cloud_components.argtypes = [vp, i64, f64, vp, sz, vp, vp]
        L.mvsdf_cloud_clean.argtypes = [vp, i64, i32, f64, f64, f64, vp, sz, vp, vp, vp, vp]
        L.mvsdf_cloud_compact.argtypes = [vp] * 5 + [i64, vp, sz] + [vp] * 4 + [i64, vp]
        L.mvsdf_raster_workspace_bytes.restype = sz
        L.mvsdf_raster_workspace_bytes.argtypes = [i64] * 5
        L.mvsdf_raster_draw.argtypes = [vp, vp, i64, i64, vp, i64, i64, i64, f64, i64, i32, vp, sz, vp]
        L.mvsdf_raster_resolve.argtypes = [i64, i64, i64, vp, sz, vp, vp, vp]
        L.mvsdf_raster_visibility.argtypes = [vp, i64, vp, i64, i64, i64, f64, vp, vp, f64, vp, sz, vp, vp]
        L.mvsdf_raster_colors.argtypes = [vp, vp, i64, vp, vp, i64, i64, i64, f64, vp, vp, vp, f64, f64, i32, f32, f32, f32, vp, sz, vp, vp, vp]
        L.mvsdf_texture_workspace_bytes.restype = sz
        L.mvsdf_texture_workspace_bytes.argtypes = [i64]
        L.mvsdf_texture_face_views.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, i64, i64, f64, vp, vp, f64, f64, i32, vp, sz, vp, vp, vp, vp]
        L.mvsdf_texture_classify.argtypes = [vp, vp, i64, f64, vp, sz, vp, vp]
        L.mvsdf_texture_pack.argtypes = [vp, i64, vp, vp, sz, vp, vp, vp, vp]
        L.mvsdf_texture_fill.argtypes = [vp, i64, i64, i64, f64, vp, vp, vp, i64, vp, vp, vp, i64, vp, i32, i32, i32, i32, i64, i64, vp, vp, vp]
        for fn in ('mvsdf_featext_raw_floats', 'mvsdf_featext_pack_bytes', 'mvsdf_featext_workspace_bytes', 'mvsdf_featext_layer_workspace_bytes'):
            getattr(L, fn).restype = sz
        L.mvsdf_featext_raw_floats.argtypes = []
        L.mvsdf_featext_pack_bytes.argtypes = []
        L.mvsdf_featext_pack.argtypes = [vp, vp, sz, vp]
        L.mvsdf_featext_workspace_bytes.argtypes = [i64] * 3
        L.mvsdf_featext_forward.argtypes = [vp, vp, i64, i64, i64, vp, sz, vp, vp, vp, C.c_int, C.c_int, vp]
        L.mvsdf_featext_layer_workspace_bytes.argtypes = [C.c_int] * 5
        L.mvsdf_featext_layer.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, i64, i64, i64, vp, C.c_int, vp, sz, vp, vp]
        for fn in ('mvsdf_stereo_workspace_bytes', 'mvsdf_stereo_volume_offset'):
            getattr(L, fn).restype = sz
            getattr(L, fn).argtypes = [i64] * 4
        L.mvsdf_stereo_normalize.argtypes = [vp, i64, i64, vp, vp, vp]
        L.mvsdf_stereo_patches.argtypes = [vp, i64, i64, i64, i32, vp, vp]
        L.mvsdf_stereo_sweep.argtypes = [vp, i64, i64, i64, i64, i64] + [vp] * 7 + [sz] + [vp] * 5
        L.mvsdf_stereo_sgm_workspace_bytes.restype = sz
        L.mvsdf_stereo_sgm_workspace_bytes.argtypes = [i64] * 3
        L.mvsdf_stereo_regularize.argtypes = [vp, i64, i64, i64, f64, f64, i32, vp, sz, vp, vp]
        L.mvsdf_stereo_sweep_sgm_workspace_bytes.restype = sz
        L.mvsdf_stereo_sweep_sgm_workspace_bytes.argtypes = [i64] * 4
        L.mvsdf_stereo_sweep_sgm.argtypes = [vp, i64, i64, i64, i64, i64] + [vp] * 6 + [f64, f64, i32, vp, sz] + [vp] * 5
        L.mvsdf_stereo_upsample.argtypes = [vp, vp] + [i64] * 5 + [vp, vp]
        L.mvsdf_stereo_band_workspace_bytes.restype = sz
        L.mvsdf_stereo_band_workspace_bytes.argtypes = [i64] * 5
        L.mvsdf_stereo_band.argtypes = [vp, i64, i64, i64, i64, i64] + [vp] * 6 + [i32, vp, sz] + [vp] * 5
        L.mvsdf_viewsel_bits_bytes.restype = sz
        L.mvsdf_viewsel_bits_bytes.argtypes = [i64, i64]
        L.mvsdf_viewsel_workspace_bytes.restype = sz
        L.mvsdf_viewsel_workspace_bytes.argtypes = [i64]
        L.mvsdf_viewsel_pack_dense.argtypes = [vp, i64, i64, vp, vp, vp]
        L.mvsdf_viewsel_pack_tracks.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp]
        L.mvsdf_viewsel_scores.argtypes = [vp, vp, vp, i64, i64, f64, f64, f64, vp, sz, vp, vp, vp, vp]
        L.mvsdf_viewsel_depths.argtypes = [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp]
        L.mvsdf_viewsel_weights_host.argtypes = [vp, vp, i64, f64, f64, f64, vp, vp]
        L.mvsdf_undistort_points.argtypes = [vp, i64, C.c_int, vp, vp, C.c_int, vp, vp, vp]
        L.mvsdf_undistort_images.argtypes = [vp, i64, i64, i64, i64, C.c_int, C.c_int, vp, vp, i64, i64, vp, vp, vp]
        L.mvsdf_undistort_points_host.argtypes = [vp, i64, C.c_int, vp, vp, C.c_int, vp, vp]
        L.mvsdf_undistort_images_host.argtypes = [vp, i64, i64, i64, i64, C.c_int, C.c_int, vp, vp, i64, i64, vp, vp]
        L.mvsdf_batch_args_bytes.restype = sz
        L.mvsdf_batch_args_bytes.argtypes = []
        L.mvsdf_batch_gather.argtypes = [vp, vp]
        for name in EXPORTS:
            getattr(L, name)
        _lib = L
    return _lib


# every symbol include/mvsdf_hip.h declares (tests/test_abi.py checks the header against this list and the .so)
EXPORTS = [
    'mvsdf_version', 'mvsdf_abi_struct_sizes', 'mvsdf_last_error', 'mvsdf_packed_floats', 'mvsdf_fold_pack', 'mvsdf_fold_backward', 'mvsdf_fold_pack_net', 'mvsdf_fold_backward_net', 'mvsdf_packed_bf16_bytes', 'mvsdf_pack_bf16w_net', 'mvsdf_pack_bf16s_net', 'mvsdf_pack_bf16x3_net', 'mvsdf_pack_bf16x3t_net',
    'mvsdf_sdf_col0', 'mvsdf_camera_rays', 'mvsdf_sphere_intersection', 'mvsdf_trace_workspace_bytes', 'mvsdf_trace_workspace_bytes_n', 'mvsdf_trace', 'mvsdf_trace_stage', 'mvsdf_trace_cut_workspace_bytes', 'mvsdf_trace_cut_stage', 'mvsdf_det_math',
    'mvsdf_tracegen_state_bytes', 'mvsdf_tracegen_init', 'mvsdf_tracegen_step', 'mvsdf_tracegen_finish', 'mvsdf_tracegen_rows', 'mvsdf_tracegen_reduce',
    'mvsdf_tracegen_secant',
    'mvsdf_sdf_ctx_floats', 'mvsdf_sdf_forward', 'mvsdf_sdf_bwd_ws_floats', 'mvsdf_sdf_backward', 'mvsdf_sdf_backward_pair', 'mvsdf_sdf_backward_finish',
    'mvsdf_feat_corr', 'mvsdf_depth_carve', 'mvsdf_loss_terms', 'mvsdf_loss_prep', 'mvsdf_loss_scale', 'mvsdf_adam_ws_floats', 'mvsdf_adam_step', 'mvsdf_adam_step_scaled', 'mvsdf_adam_step_fused',
    'mvsdf_partition_rays', 'mvsdf_step_outputs', 'mvsdf_step_backward_inputs', 'mvsdf_step_backward_fbar', 'mvsdf_dsurf_select', 'mvsdf_dsurf_points',
    'mvsdf_render_ctx_floats', 'mvsdf_render_bwd_ws_floats', 'mvsdf_render_forward', 'mvsdf_render_backward',
    'mvsdf_step_create', 'mvsdf_step_destroy', 'mvsdf_step_forward', 'mvsdf_step_resolve_unhit', 'mvsdf_step_can_defer_unhit', 'mvsdf_step_set_sphere_cut', 'mvsdf_step_last_tracer_grid', 'mvsdf_step_wait_counts', 'mvsdf_step_backward', 'mvsdf_step_set_timing', 'mvsdf_step_trace_times', 'mvsdf_step_times',
    'mvsdf_step_seq', 'mvsdf_step_counts_offset', 'mvsdf_step_wait_counts_seq', 'mvsdf_step_done_seq', 'mvsdf_step_can_defer', 'mvsdf_step_saved_offsets', 'mvsdf_step_pack_offsets',
    'mvsdf_loss_layout', 'mvsdf_loss_forward', 'mvsdf_loss_backward',
    'mvsdf_mc_workspace_bytes', 'mvsdf_mc_count', 'mvsdf_mc_emit', 'mvsdf_mesh_cc_workspace_bytes', 'mvsdf_mesh_components', 'mvsdf_mesh_select',
    'mvsdf_smc_workspace_bytes', 'mvsdf_smc_emit_workspace_bytes', 'mvsdf_smc_coarse_points', 'mvsdf_smc_seed', 'mvsdf_smc_brick_points',
    'mvsdf_smc_closure', 'mvsdf_smc_count', 'mvsdf_smc_emit',
    'mvsdf_mesh_cut_workspace_bytes', 'mvsdf_mesh_cut', 'mvsdf_mesh_trim',
    'mvsdf_mesh_simplify_workspace_bytes', 'mvsdf_mesh_simplify', 'mvsdf_mesh_simplify_emit',
    'mvsdf_chamfer_key', 'mvsdf_chamfer_sample_workspace_bytes', 'mvsdf_chamfer_sample_count', 'mvsdf_chamfer_sample_emit',
    'mvsdf_chamfer_downsample_workspace_bytes', 'mvsdf_chamfer_downsample', 'mvsdf_chamfer_mask_workspace_bytes', 'mvsdf_chamfer_mask',
    'mvsdf_chamfer_nearest_workspace_bytes', 'mvsdf_chamfer_nearest',
    'mvsdf_fusion_workspace_bytes', 'mvsdf_fusion_fuse', 'mvsdf_fusion_emit', 'mvsdf_fusion_normals_workspace_bytes', 'mvsdf_fusion_normals',
    'mvsdf_poisson_workspace_bytes', 'mvsdf_poisson_reconstruct', 'mvsdf_poisson_valid', 'mvsdf_poisson_volume',
    'mvsdf_tsdf_workspace_bytes', 'mvsdf_tsdf_integrate', 'mvsdf_mcm_workspace_bytes', 'mvsdf_mcm_count', 'mvsdf_mcm_emit',
    'mvsdf_cloud_clean_workspace_bytes', 'mvsdf_cloud_compact_workspace_bytes', 'mvsdf_cloud_knn', 'mvsdf_cloud_components', 'mvsdf_cloud_clean',
    'mvsdf_cloud_compact',
    'mvsdf_raster_workspace_bytes', 'mvsdf_raster_draw', 'mvsdf_raster_resolve', 'mvsdf_raster_visibility', 'mvsdf_raster_colors',
    'mvsdf_texture_workspace_bytes', 'mvsdf_texture_face_views', 'mvsdf_texture_classify', 'mvsdf_texture_pack',
    'mvsdf_texture_fill',
    'mvsdf_featext_raw_floats', 'mvsdf_featext_pack_bytes', 'mvsdf_featext_pack', 'mvsdf_featext_workspace_bytes', 'mvsdf_featext_forward',
    'mvsdf_featext_layer_workspace_bytes', 'mvsdf_featext_layer',
    'mvsdf_stereo_workspace_bytes', 'mvsdf_stereo_volume_offset', 'mvsdf_stereo_normalize', 'mvsdf_stereo_patches', 'mvsdf_stereo_sweep',
    'mvsdf_stereo_sgm_workspace_bytes', 'mvsdf_stereo_regularize', 'mvsdf_stereo_sweep_sgm_workspace_bytes', 'mvsdf_stereo_sweep_sgm',
    'mvsdf_stereo_upsample', 'mvsdf_stereo_band_workspace_bytes', 'mvsdf_stereo_band',
    'mvsdf_viewsel_bits_bytes', 'mvsdf_viewsel_workspace_bytes', 'mvsdf_viewsel_pack_dense', 'mvsdf_viewsel_pack_tracks', 'mvsdf_viewsel_scores',
    'mvsdf_viewsel_depths', 'mvsdf_viewsel_weights_host',
    'mvsdf_undistort_points', 'mvsdf_undistort_images', 'mvsdf_undistort_points_host', 'mvsdf_undistort_images_host',
    'mvsdf_batch_args_bytes', 'mvsdf_batch_gather',
]


def check(rc, what=''):
    if rc != 0:
        raise MvsdfError('%s failed (code %d): %s' % (what or 'mvsdf call', rc, lib().mvsdf_last_error().decode()))


def ptr(t):
    """device (or host) pointer of a contiguous torch tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return C.c_void_p(t.data_ptr())


def stream_of(t):
    import torch
    if t.is_cuda:
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return C.c_void_p(0)


# what the scene-side modules (mesh, chamfer, cloud, fusion, raster, stereo, viewsel) pass to their calls: raw addresses, no contiguity check
def _vp(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _header(ws, n):
    """the int64 results a call leaves at the start of its workspace (reading them waits for the stream)"""
    import torch
    return [int(x) for x in ws[:8 * n].view(torch.int64).cpu()]


def f64_from_bits(bits):
    """the fp64 value a header word holds as its int64 bit pattern"""
    return struct.unpack('<d', struct.pack('<q', bits))[0]
