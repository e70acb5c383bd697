"""ctypes loader of the C-ABI library (include/g4s_rasterizer.h, include/g4s_render_maps.h).

There is deliberately NO fallback: if libg4s_hip.so is missing or fails to load, importing the
operators raises.  The product path never routes through the CPU oracle or any torch emulation."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libg4s_hip.so")

RESIZE_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)

c_f = ctypes.c_float
c_i = ctypes.c_int
c_p = ctypes.c_void_p
c_sz = ctypes.c_size_t


class G4sPackedRows(ctypes.Structure):  # g4s_packed_rows
    _fields_ = [("rows", ctypes.c_void_p), ("block_offs", ctypes.c_void_p), ("capacity", ctypes.c_longlong)]


class G4sChartDeformShape(ctypes.Structure):  # g4s_chart_deform_shape
    _fields_ = [("n", ctypes.c_int), ("height", ctypes.c_int), ("width", ctypes.c_int), ("levels", ctypes.c_int),
                ("channels", ctypes.c_int), ("level_height", ctypes.c_int * 8), ("level_width", ctypes.c_int * 8),
                ("bins", ctypes.c_int), ("layers", ctypes.c_int), ("layer_size", ctypes.c_int), ("scene_radius", ctypes.c_float),
                ("deformation_radius", ctypes.c_float)]


class G4sLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in (
        "rec", "clamped", "depth_sorted", "tiles_touched", "geom_bytes", "entries", "qhit", "binning_bytes", "ranges",
        "final_T", "n_contrib", "tile_order", "image_bytes", "hot_count")]


# symbol -> (restype, argtypes); tests/test_abi.py checks this table against include/g4s_rasterizer.h
SIGNATURES = {
    "g4s_last_error": (ctypes.c_char_p, []),
    "g4s_version": (ctypes.c_char_p, []),
    "g4s_rasterizer_forward": (c_i, [RESIZE_FN, c_p, RESIZE_FN, c_p, RESIZE_FN, c_p, c_i, c_i, c_i, c_p, c_i, c_i,
                                     c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_i, c_p, c_p,
                                     c_p, c_i, c_p]),
    "g4s_rasterizer_backward_workspace": (c_sz, [c_i, c_i]),
    "g4s_rasterizer_backward": (c_i, [c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p,
                                      c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                      c_p, c_p, c_p, c_sz, c_i, c_p]),
    "g4s_rasterizer_forward_split_sh": (c_i, [RESIZE_FN, c_p, RESIZE_FN, c_p, RESIZE_FN, c_p, c_i, c_i, c_i, c_p, c_i,
                                              c_i, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_i,
                                              c_p, c_p, c_p, c_i, c_p]),
    "g4s_rasterizer_backward_split_sh": (c_i, [c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p,
                                               c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                               c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_p]),
    "g4s_rasterizer_backward_accumulate": (c_i, [c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p,
                                                 c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                                 c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p, c_i, c_p]),
    "g4s_rasterizer_backward_accumulate_packed": (c_i, [c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p,
                                                        c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                                        c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_sz, c_p, c_i, c_p]),
    "g4s_rasterizer_forward_presized": (c_i, [c_p, c_sz, c_p, c_sz, c_p, c_sz, c_i, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p,
                                              c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_p, c_p, c_p, c_i,
                                              c_p]),
    "g4s_rasterizer_mark_visible": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p]),
    "g4s_knn_workspace": (c_sz, [c_i]),
    "g4s_knn_mean_dist": (c_i, [c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_rasterizer_layout": (c_i, [c_i, c_i, c_i, c_i, ctypes.POINTER(G4sLayout)]),
    "g4s_set_option": (c_i, [ctypes.c_char_p, c_i]),
    "g4s_get_option": (c_i, [ctypes.c_char_p, ctypes.POINTER(c_i)]),
    "g4s_pack_rows": (c_i, [c_i, c_p, c_p, c_p, c_i, c_p, c_i, c_p]),
    "g4s_accumulate_rows": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p]),
    "g4s_accumulate_rows_ordered": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p]),
    "g4s_profile_enable": (None, [c_i]),
    "g4s_profile_kernels": (c_i, []),
    "g4s_profile_name": (ctypes.c_char_p, [c_i]),
    "g4s_profile_read": (c_i, [c_i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i)]),
    "g4s_profile_reset": (None, []),
    # include/g4s_optim.h
    "g4s_adam_step": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_p]),
    "g4s_adam_step_device": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   c_p]),
    "g4s_densify_stats": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_activations_forward": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_activations_backward": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_activations_mip_forward": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_activations_mip_backward": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_mip_filter_workspace": (c_sz, []),
    "g4s_mip_filter": (c_i, [c_i, c_p, c_i, c_p, c_f, c_f, c_p, c_p, c_p]),
    "g4s_compact_workspace": (c_sz, [c_i]),
    "g4s_compact_scan": (c_i, [c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_compact_gather": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, c_p, ctypes.c_longlong, c_p]),
    # include/g4s_losses.h
    "g4s_photometric_workspace": (c_sz, [c_i, c_i]),
    "g4s_photometric_loss": (c_i, [c_i, c_i, c_p, c_p, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_geometry_regularizers_workspace": (c_sz, [c_i, c_i]),
    "g4s_geometry_regularizers_forward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_geometry_regularizers_backward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_chart_prior_workspace": (c_sz, [c_i, c_i]),
    "g4s_chart_prior_forward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_prior_backward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p,
                                       c_sz, c_p]),
    "g4s_anisotropy_workspace": (c_sz, [c_i]),
    "g4s_anisotropy_forward": (c_i, [c_i, c_p, c_f, c_p, c_p, c_sz, c_p]),
    "g4s_anisotropy_backward": (c_i, [c_i, c_p, c_f, c_p, c_p, c_p]),
    "g4s_chart_match_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_chart_match": (c_i, [c_i, c_i, c_i, c_p, c_p, c_f, c_p, c_p, c_i, c_p, c_p]),
    "g4s_chart_match_loss_forward": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_sz, c_p]),
    "g4s_chart_match_loss_backward": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_align_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_chart_align_normals": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "g4s_chart_align_forward": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_chart_align_backward": (c_i, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_i, c_p, c_p, c_p, c_p,
                                       c_sz, c_p]),
    "g4s_chart_deform_workspace": (c_sz, [ctypes.POINTER(G4sChartDeformShape)]),
    "g4s_chart_deform_forward": (c_i, [ctypes.POINTER(G4sChartDeformShape), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                       c_p]),
    "g4s_chart_deform_backward": (c_i, [ctypes.POINTER(G4sChartDeformShape), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                        c_p, c_p, c_sz, c_p]),
    "g4s_chart_confidence_forward": (c_i, [ctypes.c_longlong, c_p, c_p, c_p, c_p]),
    "g4s_chart_confidence_backward": (c_i, [ctypes.c_longlong, c_p, c_p, c_p, c_p]),
    "g4s_chart_deform_reg_workspace": (c_sz, [ctypes.POINTER(G4sChartDeformShape), c_i]),
    "g4s_chart_deform_reg_forward_workspace": (c_sz, [ctypes.POINTER(G4sChartDeformShape), c_i]),
    "g4s_chart_deform_reg_forward": (c_i, [ctypes.POINTER(G4sChartDeformShape), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p,
                                           c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_deform_reg_backward": (c_i, [ctypes.POINTER(G4sChartDeformShape), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p,
                                            c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_points_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "g4s_chart_points_index_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "g4s_chart_points_project": (c_i, [c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_chart_points_sample": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    "g4s_chart_points_fit": (c_i, [c_i, c_i, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_points_apply": (c_i, [c_i, c_i, c_i, c_p, c_p, c_f, c_p, c_p]),
    "g4s_chart_points_view_depths": (c_i, [c_i, c_p, ctypes.c_longlong, ctypes.c_longlong, c_p, c_p, c_f, c_p, c_p]),
    "g4s_chart_points_index": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_points_loss_forward": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_sz, c_p]),
    "g4s_chart_points_loss_backward": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                             c_p]),
    "g4s_chart_points_sample_backward": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]),
    # include/g4s_render_maps.h
    "g4s_render_maps_workspace": (c_sz, []),
    "g4s_render_maps_forward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                      c_p]),
    "g4s_render_maps_backward": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                       c_p, c_sz, c_p]),
    "g4s_tsdf_blocks_per_pixel": (c_i, [c_i, c_i, c_p, c_f, c_f]),
    "g4s_tsdf_workspace": (c_sz, [c_i, c_i, c_i, c_i]),
    "g4s_tsdf_alloc_count": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_tsdf_merge": (c_i, [c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_sz, c_p]),
    "g4s_tsdf_integrate": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_sz,
                                 c_p]),
    "g4s_tsdf_extract_count": (c_i, [c_p, c_p, c_i, c_p, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_tsdf_extract_emit": (c_i, [c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_f, c_p, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "g4s_utsdf_workspace": (c_sz, [c_i]),
    "g4s_utsdf_grid": (c_i, [c_i, c_f, c_p, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_utsdf_sample": (c_i, [c_i, c_p, c_i, c_p, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_dense_mc_workspace": (c_sz, [c_i]),
    "g4s_dense_mc_count": (c_i, [c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_dense_mc_emit": (c_i, [c_i, c_p, c_f, c_p, c_f, c_f, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "g4s_atsdf_workspace": (c_sz, [c_i]),
    "g4s_atsdf_sample": (c_i, [c_i, c_p, c_f, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_atsdf_bisect": (c_i, [c_i, c_p, c_i, c_p, c_p, c_i, c_f, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_mtet_workspace": (c_sz, [c_i]),
    "g4s_mtet_count": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_mtet_emit": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "g4s_mesh_observed_vertices": (c_i, [c_i, c_p, c_i, c_p, c_p, c_f, c_p, c_p]),
    "g4s_mesh_keep_unobserved": (c_i, [c_i, c_p, c_i, c_p, c_p, c_p]),
    "g4s_mesh_keep_min_size": (c_i, [c_i, c_p, c_i, c_p, c_p]),
    "g4s_mesh_keep_nondegenerate": (c_i, [c_i, c_p, c_p, c_p]),
    "g4s_mesh_keep_short_edges": (c_i, [c_i, c_p, c_i, c_p, ctypes.c_double, c_p, c_p]),
    "g4s_mesh_cluster_workspace": (c_sz, [c_i]),
    "g4s_mesh_cluster_triangles": (c_i, [c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_mesh_compact_workspace": (c_sz, [c_i, c_i]),
    "g4s_mesh_compact_count": (c_i, [c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_mesh_compact_emit": (c_i, [c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "g4s_nn_workspace": (c_sz, [c_i, c_i]),
    "g4s_nn_search": (c_i, [c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_voxel_downsample_workspace": (c_sz, [c_i]),
    "g4s_voxel_downsample_count": (c_i, [c_i, c_p, c_f, c_p, c_p, c_sz, c_p]),
    "g4s_voxel_downsample_emit": (c_i, [c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_mesh_sample_surface": (c_i, [c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p]),
    "g4s_visgrid_workspace": (c_sz, [c_i]),
    "g4s_visgrid_build": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_sample": (c_i, [c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_march": (c_i, [c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_march_bytes": (c_i, [c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_expand": (c_i, [c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_compact_workspace": (c_sz, [c_i]),
    "g4s_visgrid_compact_count": (c_i, [c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_visgrid_compact_emit": (c_i, [c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_view_counts_points": (c_i, [c_i, c_p, c_i, c_f, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_view_counts_pixels": (c_i, [c_i, c_i, c_p, c_p, c_i, c_f, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_to_points": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_labels_workspace": (c_sz, [c_i, c_p]),
    "g4s_plane_labels": (c_i, [c_i, c_p, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_overlap": (c_i, [c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_assign_workspace": (c_sz, [c_i]),
    "g4s_plane_assign": (c_i, [c_i, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_plane_row_overlap": (c_i, [c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_plane_row_merge": (c_i, [c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_sz, c_p]),
    "g4s_plane_row_mask": (c_i, [c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_consistency_points_workspace": (c_sz, [c_i, c_i, c_p]),
    "g4s_consistency_points": (c_i, [c_i, c_p, c_f, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_sz,
                                     c_p]),
    "g4s_consistency_plane_counts_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_consistency_plane_counts": (c_i, [c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_sz,
                                           c_p]),
    "g4s_consistency_plane_repaint_workspace": (c_sz, [c_i, c_p, c_i]),
    "g4s_consistency_plane_repaint": (c_i, [c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_view_bits_workspace": (c_sz, [c_i]),
    "g4s_view_bits": (c_i, [c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_view_overlap": (c_i, [c_i, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_fps_workspace": (c_sz, [c_i, c_i]),
    "g4s_fps": (c_i, [c_i, c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_align_workspace": (c_sz, [c_i, c_p]),
    "g4s_depth_align": (c_i, [c_i, c_i, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_align_apply_workspace": (c_sz, [c_i]),
    "g4s_depth_align_apply": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_cue_maps_workspace": (c_sz, [c_i]),
    "g4s_depth_cue_maps": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_depths_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_plane_depths": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_refill_workspace": (c_sz, [c_i]),
    "g4s_depth_refill": (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_chart_surfels_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_chart_surfels_count": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_f, c_p, c_p, c_sz, c_p]),
    "g4s_chart_surfels_emit": (c_i, [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_f, c_f, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_voxel_downsample_emit_index": (c_i, [c_i, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_warp_init_workspace": (c_sz, [c_i, c_p, c_i]),
    "g4s_warp_init_count": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_warp_init_emit": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_kmeans_normals_workspace": (c_sz, [c_i, c_p]),
    "g4s_kmeans_normals": (c_i, [c_i, c_p, c_p, c_i, c_p, c_i, ctypes.c_double, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_normal_components_workspace": (c_sz, [c_i, c_p]),
    "g4s_normal_components_count": (c_i, [c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_normal_components_sizes": (c_i, [c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_pair_counts_workspace": (c_sz, [c_i]),
    "g4s_plane_pair_counts": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_paint_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_plane_paint": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_relabel_workspace": (c_sz, [c_i, c_i]),
    "g4s_plane_relabel": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_gather_workspace": (c_sz, [c_i, c_p, c_i, c_p]),
    "g4s_plane_fit_gather_count": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_gather_emit": (c_i, [c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, ctypes.c_longlong, c_p, c_p,
                                        c_p, c_sz, c_p]),
    "g4s_plane_fit_members_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_plane_fit_members_count": (c_i, [c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_members_emit": (c_i, [c_i, c_i, c_i, c_p, c_i, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_workspace": (c_sz, [c_i, c_p]),
    "g4s_plane_fit_hypotheses": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, ctypes.c_double, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_score": (c_i, [c_i, c_p, c_p, c_i, c_p, ctypes.c_double, c_p, c_p, c_sz, c_p]),
    "g4s_plane_fit_refit": (c_i, [c_i, c_p, c_p, c_i, c_p, c_p, ctypes.c_double, c_p, ctypes.c_double, c_p, c_p, c_p, c_p, c_sz,
                                  c_p]),
    "g4s_mesh_raster_workspace": (c_sz, [c_i, c_i, c_i]),
    "g4s_mesh_raster": (c_i, [c_i, c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_i, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p,
                              c_p, c_p, c_p, c_sz, c_p]),
    "g4s_depth_dilate_workspace": (c_sz, [c_i, c_p]),
    "g4s_depth_dilate": (c_i, [c_i, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_p, c_p, c_p, c_sz, c_p]),
}

_lib = None


def load():
    """Load libg4s_hip.so and bind every exported symbol.  Raises RuntimeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # torch-ROCm bundles its own HIP runtime (same SONAME as /opt/rocm's).  It must be the one
    # already resident when libg4s_hip.so is mapped, otherwise two runtimes end up in the process
    # and torch's stream / memory handles are meaningless to ours.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m g4splat_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().g4s_last_error().decode()


# ---- argument helpers of the library calls -----------------------------------------------------------------------
def ptr(t):
    """A tensor's device address as a `void*` argument (None -> NULL)."""
    return c_p(t.data_ptr() if t is not None else 0)


def ptrs(tensors):
    """HOST array of the tensors' device addresses (None -> NULL)."""
    return (c_p * len(tensors))(*[t.data_ptr() if t is not None else 0 for t in tensors])


def array(ctype, values):
    """HOST array of `ctype` (c_int, ctypes.c_longlong, ctypes.c_double, ...) from a list."""
    return (ctype * len(values))(*values)


def stream(dev):
    """The current torch stream of device `dev` as the `void* stream` argument."""
    import torch
    return c_p(torch.cuda.current_stream(dev).cuda_stream)


def call(name, *args):
    """lib.<name>(*args); a non-zero status raises RuntimeError with the library's last error."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {last_error()}")


OPTION_UNSET = -2147483648  # G4S_OPTION_UNSET


def set_option(name, value):
    """Diagnostic switch of the library (include/g4s_rasterizer.h: g4s_set_option).  The library never reads the
    environment on a call path; the parity tests flip these instead."""
    if load().g4s_set_option(name.encode(), int(value)) != 0:
        raise ValueError(last_error())


def get_option(name):
    v = c_i(0)
    if load().g4s_get_option(name.encode(), ctypes.byref(v)) != 0:
        raise ValueError(last_error())
    return v.value


class option:
    """`with _lib.option("no_fastpath", 1): ...` -- sets a diagnostic switch and restores its previous value."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.prev)
        return False
