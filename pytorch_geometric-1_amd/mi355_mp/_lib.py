"""ctypes binding of the C-ABI in include/mi355_mp.h (libmi355_mp.so).

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C pytorch_geometric-1_amd/csrc``).  There is no fallback: if the
library is missing, or a tensor is not on a ROCm device, every op raises.
Only plain pointers, sizes and the HIP stream handle cross the boundary.
"""
import ctypes
import os
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "libmi355_mp.so")
LIB_PATH = os.environ.get("MI355_MP_LIB", DEFAULT_LIB_PATH)

MP_OK = 0
MP_REDUCE = {"sum": 0, "add": 0, "mean": 1, "max": 2, "min": 3}
MP_FLAG_INIT_FROM_OUT = 1
MP_FLAG_PYG_MASK = 2
MP_FLAG_SKIP_EMPTY = 4
MP_STAGE_MAIN = 1
MP_STAGE_FIXUP = 2
MP_STAGE_STATS = 4
MP_STAGE_ALL = 7
MP_TUNE_FLAT_VEC1_MIN_BYTES = 1
MP_TUNE_FLAT_SMEM = 2
MP_TUNE_FLAT_MIN_F = 3
MP_TUNE_FLAT_MIN_F_ARG = 4
MP_TUNE_FLAT_NARROW_VEC1 = 5
MP_TUNE_FLAT_VEC = 6
MP_TUNE_FLAT_VEC_ARG = 7
MP_TUNE_FLAT_SEQ_TILES = 8
MP_TUNE_FLAT_FAR_MIN_BYTES = 9
MP_TUNE_GAT_BWD_VEC = 10
MP_TUNE_TOPK_WG_LIMIT = 11
MP_POOL_SCORE_TANH = 1
MP_POOL_SCORE_RAW = 2
MP_DTYPE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int64: 4}
MP_LOOPS_REMOVE = 0
MP_LOOPS_ADD = 1
MP_LOOPS_ADD_REMAINING = 2

c_p = ctypes.c_void_p
i64 = ctypes.c_int64
u64 = ctypes.c_uint64
i32 = ctypes.c_int32
f32 = ctypes.c_float
sz = ctypes.c_size_t


class MpCsr(ctypes.Structure):
    _fields_ = [
        ("rowptr", c_p), ("col", c_p), ("eid", c_p), ("wave_row", c_p),
        ("wave_slot", c_p), ("split_waves", c_p), ("n_rows", i64),
        ("n_edges", i64), ("chunk", i32), ("n_waves", i32), ("n_split", i32),
        ("n_cols", i32), ("n_ids", i64),
    ]


# name -> (restype, argtypes); mirrors include/mi355_mp.h one to one.
SIGNATURES = {
    "mp_last_error": (ctypes.c_char_p, []),
    "mp_abi_version": (ctypes.c_int, []),
    "mp_source_hash": (ctypes.c_char_p, []),
    "mp_tune": (i64, [i32, i64]),
    "mp_csr_build_workspace": (sz, [i64, i64]),
    "mp_csr_build": (ctypes.c_int, [c_p, c_p, i64, i64, i64, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "mp_schedule_n_waves": (i32, [i64, i64, i32]),
    "mp_schedule_workspace": (sz, [i32]),
    "mp_schedule_build": (ctypes.c_int, [c_p, i64, i64, i32, i32, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "mp_aggregate_slab_bytes": (sz, [ctypes.POINTER(MpCsr), i32, i32]),
    "mp_aggregate_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i64, i32, i32, i32, c_p,
                                        c_p, i64, c_p, c_p, sz, i32, c_p]),
    "mp_aggregate_kernel_name": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i64, i32, i32, c_p, c_p, i64,
                                                ctypes.c_char_p, sz, c_p]),
    "mp_gat_node_scores_f32": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, c_p, c_p]),
    "mp_gat_slab_bytes": (sz, [ctypes.POINTER(MpCsr), i32, i32]),
    "mp_gat_aggregate_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, i32, i32, f32, c_p,
                                            c_p, i64, c_p, c_p, sz, i32, c_p]),
    "mp_gat_aggregate_att_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, c_p, i32, i32, f32, c_p,
                                                c_p, i64, c_p, c_p, sz, i32, c_p]),
    "mp_gat_forward_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i32, i32, f32, c_p, c_p, i64, c_p, c_p,
                                          c_p, c_p, sz, i32, c_p]),
    "mp_gat_forward_train_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i32, i32, f32, c_p, c_p, i64, c_p,
                                                c_p, c_p, c_p, c_p, c_p, c_p, sz, i32, c_p]),
    "mp_gat_train_ok": (ctypes.c_int, [i32, i32]),
    "mp_gat_train_slab_bytes": (sz, [ctypes.POINTER(MpCsr), i32, i32]),
    "mp_gat_aggregate_train_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, c_p, i32, i32, f32,
                                                  c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, sz, i32, c_p]),
    "mp_gat_two_pass_ok": (ctypes.c_int, [i32, i32]),
    "mp_gat_softmax_aggregate_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, c_p, i32, i32, f32,
                                                    c_p, c_p, i64, c_p, c_p, sz, i32, c_p]),
    "mp_gat_alpha_f32": (ctypes.c_int, [c_p, c_p, i64, i32, c_p, c_p, f32, c_p, c_p, c_p]),
    "mp_csr_slot_rows": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p]),
    "mp_gat_alpha_csr_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, i32, f32, c_p, c_p, c_p,
                                            c_p]),
    "mp_aggregate_heads_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i32, c_p, i64, i32, c_p, i64, c_p,
                                              sz, i32, c_p]),
    "mp_gat_sddmm_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i64, c_p, i64, i32, i32, c_p, c_p]),
    "mp_gat_backward_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, c_p, c_p, c_p, c_p, i32, i32,
                                           ctypes.c_float, c_p, c_p, c_p, sz, c_p, sz, i32, c_p]),
    "mp_gat_backward_train_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, c_p, c_p, c_p, c_p, i32, i32,
                                                 ctypes.c_float, c_p, c_p, c_p, c_p, sz, i32, c_p]),
    "mp_gat_aggregate_train_drop_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, c_p, c_p, i32, i32, f32,
                                                       c_p, c_p, i64, c_p, c_p, c_p, c_p, u64, f32, c_p, c_p, sz, i32,
                                                       c_p]),
    "mp_gat_backward_train_drop_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, c_p, c_p, c_p, c_p, i32,
                                                      i32, f32, c_p, u64, f32, c_p, c_p, c_p, c_p, sz, i32, c_p]),
    "mp_gat_dropout_keep": (ctypes.c_int, [u64, f32, i32, i64, c_p, c_p, c_p]),
    "mp_gat_wide_ok": (ctypes.c_int, [i32, i32]),
    "mp_gat_node_scores_wide_f32": (ctypes.c_int, [c_p, i64, i32, i32, c_p, c_p, c_p, c_p]),
    "mp_gat_backward_prep_wide_f32": (ctypes.c_int, [c_p, i64, c_p, i64, c_p, c_p, c_p, c_p, c_p, i64, i32, i32, c_p,
                                                     sz, c_p, c_p]),
    "mp_gat_backward_wide_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, c_p, c_p, i32, i32, f32, u64, f32, c_p,
                                                c_p, c_p, sz, c_p, sz, c_p, sz, i32, c_p]),
    "mp_gat_backward_epilogue_wide_f32": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, i64, i32, i32, c_p]),
    "mp_segment_offset_i64": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, i64, c_p]),
    "mp_segment_ids_i64": (ctypes.c_int, [c_p, i64, c_p, i64, c_p]),
    "mp_gat_backward_prep_f32": (ctypes.c_int, [c_p, i64, c_p, i64, c_p, c_p, c_p, i64, i32, i32, c_p, sz, c_p, sz,
                                                c_p]),
    "mp_gat_backward_prep_train_f32": (ctypes.c_int, [c_p, i64, c_p, i64, c_p, c_p, c_p, c_p, c_p, i64, i32, i32,
                                                      c_p, sz, c_p, sz, c_p, c_p]),
    "mp_gat_bwd_blocks": (ctypes.c_int, [i64]),
    "mp_col_sums_f32": (ctypes.c_int, [c_p, i64, i64, i32, c_p, sz, c_p]),
    "mp_gemm_rows_f32": (ctypes.c_int, [c_p, i64, i64, i32, c_p, i32, i32, c_p, i64, i32, c_p]),
    "mp_gat_backward_finish_f32": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, i64, i32, i32, c_p, sz, c_p]),
    "mp_gat_merge_partials_f32": (ctypes.c_int, [i64, i32, i32, c_p, c_p, i64, c_p, sz, i64, c_p, sz, c_p, c_p, i64,
                                                 c_p, c_p, c_p, c_p]),
    "mp_aggregate_tiles_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p, i64, i32, i64, i32, i32, i32, c_p,
                                              c_p, c_p, i64, i32, i64, c_p, sz, i32, c_p]),
    "mp_heads_outer_add_f32": (ctypes.c_int, [c_p, i64, c_p, i64, i32, i32, c_p, i64, c_p]),
    "mp_gather_rows_f32": (ctypes.c_int, [c_p, i64, c_p, i64, i32, c_p, i64, c_p]),
    "mp_permute_f32": (ctypes.c_int, [c_p, c_p, i64, c_p, c_p]),
    "mp_scatter_arg_backward_f32": (ctypes.c_int, [c_p, c_p, i64, i32, i64, c_p, i64, c_p]),
    "mp_self_loop_count": (ctypes.c_int, [c_p, c_p, i64, i64, c_p, c_p]),
    "mp_self_loops_workspace": (sz, [i64, i64]),
    "mp_self_loops": (ctypes.c_int, [c_p, c_p, i64, i64, i32, i64, c_p, c_p, c_p, c_p, sz, c_p]),
    "mp_gather_fill_f32": (ctypes.c_int, [c_p, c_p, i64, f32, c_p, c_p]),
    "mp_shard_plan_workspace": (sz, [i64, i64]),
    "mp_shard_plan": (ctypes.c_int, [c_p, c_p, i64, i64, c_p, i32, i32, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p, sz,
                                     c_p]),
    "mp_gcn_norm_f32": (ctypes.c_int, [c_p, c_p, c_p, i64, i64, c_p, c_p, c_p]),
    "mp_gcn_norm_from_deg_f32": (ctypes.c_int, [c_p, c_p, c_p, i64, i64, c_p, c_p, c_p]),
    "mp_segment_sum_serial_f32": (ctypes.c_int, [c_p, c_p, c_p, i64, c_p, c_p]),
    "mp_csr_inverse_eid": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, c_p]),
    "mp_arg_mask_words": (i32, [i32]),
    "mp_arg_winner_mask": (ctypes.c_int, [c_p, i64, i32, i64, c_p, c_p, sz, c_p]),
    "mp_scatter_arg_backward_csr_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, sz, c_p, i64, i32, c_p, c_p, i64,
                                                       c_p]),
    "mp_scatter_arg_grad_w_f32": (ctypes.c_int, [c_p, c_p, i64, c_p, c_p, sz, i32, c_p, i64, c_p, i64, c_p, c_p]),
    "mp_segment_reduce": (ctypes.c_int, [ctypes.POINTER(MpCsr), i32, c_p, i64, i32, i32, i32, c_p, i64, c_p, c_p]),
    "mp_gather_rows_any": (ctypes.c_int, [i32, c_p, i64, c_p, i64, i32, c_p, i64, c_p]),
    "mp_scatter_arg_any": (ctypes.c_int, [i32, c_p, c_p, i64, i32, i64, c_p, i64, c_p]),
    "mp_spline_ok": (ctypes.c_int, [i32, i32, c_p, c_p, i32]),
    "mp_spline_basis_f32": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, i32, c_p, sz, c_p, sz, c_p]),
    "mp_spline_aggregate_bins_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, i32, c_p, c_p, i32, c_p, i64,
                                                    i32, c_p, c_p, i64, c_p]),
    "mp_spline_aggregate_gather_f32": (ctypes.c_int, [ctypes.POINTER(MpCsr), c_p, i64, i32, c_p, c_p, i32, c_p, i64,
                                                      i32, c_p, c_p, c_p, i64, c_p]),
    "mp_topk_path": (ctypes.c_int, [i64]),
    "mp_batch_stats": (ctypes.c_int, [c_p, i64, c_p, sz, c_p]),
    "mp_batch_starts": (ctypes.c_int, [c_p, i64, i64, c_p, sz, c_p]),
    "mp_pool_score_f32": (ctypes.c_int, [c_p, i64, i64, i32, c_p, i32, c_p, sz, c_p]),
    "mp_pool_score_bwd_parts": (i32, [i64]),
    "mp_pool_score_bwd_workspace": (sz, [i64, i32]),
    "mp_pool_score_bwd_f32": (ctypes.c_int, [c_p, i64, i64, i32, c_p, i32, c_p, c_p, c_p, i64, c_p, sz, c_p, sz,
                                             c_p]),
    "mp_topk_counts": (ctypes.c_int, [c_p, i64, f32, i64, c_p, sz, c_p, c_p]),
    "mp_topk_workspace": (sz, [i64, i64, i64]),
    "mp_topk_select_f32": (ctypes.c_int, [c_p, i64, c_p, i64, i64, f32, c_p, sz, c_p, sz, c_p, sz, c_p, c_p, sz,
                                          c_p]),
    "mp_pool_gate_f32": (ctypes.c_int, [c_p, i64, c_p, c_p, c_p, i64, i64, i32, f32, c_p, i64, sz, c_p, c_p, c_p]),
    "mp_pool_gate_bwd_f32": (ctypes.c_int, [c_p, i64, c_p, c_p, i64, c_p, c_p, i64, i64, i32, f32, c_p, i64, sz,
                                            c_p, sz, c_p]),
    "mp_pool_inverse": (ctypes.c_int, [c_p, i64, c_p, i64, c_p, sz, c_p]),
    "mp_pool_compact_workspace": (sz, [i64]),
    "mp_pool_compact": (ctypes.c_int, [c_p, i64, c_p, sz, c_p, c_p, sz, c_p]),
    "mp_pool_filter_workspace": (sz, [i64]),
    "mp_pool_filter_adj": (ctypes.c_int, [c_p, c_p, i64, c_p, i64, c_p, c_p, c_p, sz, c_p, c_p, sz, c_p]),
    "mp_cluster_max_blocks": (i32, []),
    "mp_voxel_keys_f32": (ctypes.c_int, [c_p, i64, i64, i32, c_p, c_p, c_p, c_p, c_p, sz, c_p]),
    "mp_cluster_build_workspace": (sz, [i64]),
    "mp_cluster_build": (ctypes.c_int, [c_p, i64, c_p, sz, c_p, sz, c_p, sz, c_p, sz, c_p, c_p, sz, c_p]),
    "mp_cluster_reduce_f32": (ctypes.c_int, [c_p, i64, i32, i32, i32, c_p, c_p, c_p, i64, c_p, i64, sz, c_p, sz,
                                             c_p, i64, i32, c_p, sz, c_p, c_p, c_p, sz, c_p]),
    "mp_cluster_edges_workspace": (sz, [i64, i64]),
    "mp_cluster_edges": (ctypes.c_int, [c_p, c_p, i64, c_p, i64, c_p, c_p, c_p, c_p, sz, c_p, sz, c_p, sz, c_p, sz,
                                        c_p]),
    "mp_cluster_edge_attr_f32": (ctypes.c_int, [c_p, i64, i32, c_p, c_p, c_p, i64, c_p, i64, sz, c_p]),
    "mp_cluster_edge_attr_bwd_f32": (ctypes.c_int, [c_p, i64, c_p, i64, i32, i64, c_p, i64, sz, c_p]),
    "mp_graclus_workspace": (sz, [i64, i64]),
    # these two return int64: a count >= 0, or -(code); the caller tests the sign (ops.graclus_match)
    "mp_graclus_init": (i64, [c_p, c_p, c_p, sz, i64, i64, u64, c_p, sz, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_graclus_rounds": (i64, [c_p, sz, c_p, sz, i64, i64, i64, i64, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_fps_path": (i64, [i64]),                  # an answer (0, 1 or 2), not a status
    "mp_fps_workspace": (sz, [i64, i64]),
    # the four calls below return int64: launches >= 0, or -(code); the caller tests the sign (ops._count_call)
    "mp_fps_f32": (i64, [c_p, i64, i64, i32, c_p, i64, i64, c_p, c_p, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_radius_workspace": (sz, [i64, i64]),
    "mp_radius_search_f32": (i64, [c_p, i64, i64, c_p, i64, i64, i32, c_p, c_p, i64, f32, i64, c_p, sz, c_p,
                                            sz, c_p]),
    "mp_radius_fill": (i64, [i64, i64, i64, c_p, c_p, sz, c_p, sz, c_p]),
    "mp_point_edge_features_f32": (i64, [c_p, i64, i32, c_p, i64, i64, c_p, i64, i64, i32, c_p, c_p, i64, c_p,
                                                  i64, sz, c_p]),
    # nearest neighbours (csrc/mp_knn.hip): int64 returns like the point-set calls, the sign tested by
    # ops._count_call; the first three answer a question (mp_knn_path: 0 or 1, or -MP_ERR_ARG)
    "mp_knn_max_k": (i64, []),
    "mp_knn_max_d": (i64, []),
    "mp_knn_path": (i64, [i32]),
    "mp_knn_workspace": (sz, [i64, i64]),
    "mp_knn_search_f32": (i64, [c_p, i64, i64, c_p, i64, i64, i32, c_p, c_p, i64, i64, c_p, sz, c_p, sz, c_p]),
    "mp_knn_fill": (i64, [i64, i64, i64, c_p, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_knn_interpolate_f32": (i64, [c_p, i64, i64, i32, i64, i64, c_p, sz, c_p, i64, sz, c_p]),
    # NNConv (csrc/mp_nnconv.hip): int64 returns like the two groups above, the sign tested by ops._count_call
    "mp_nnconv_ok": (i64, [i32, i32, i32]),        # an answer (0 or 1), not a status
    "mp_nnconv_edge_grad_width": (i64, [i32, i32]),  # an answer (0, 32 or 64), or -MP_ERR_ARG
    "mp_nnconv_aggregate_bins_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, i64, i32, c_p, i64, i32, c_p, c_p, i64,
                                           c_p]),
    "mp_nnconv_aggregate_gather_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, i64, i32, c_p, i64, i32, c_p, c_p, c_p,
                                             i64, c_p]),
    "mp_nnconv_edge_grad_f32": (i64, [c_p, c_p, i64, c_p, i64, c_p, i64, i32, i32, c_p, i64, sz, c_p]),
    # GMMConv (csrc/mp_gmm.hip): int64 returns like NNConv's, the sign tested by ops._count_call
    "mp_gmm_ok": (i64, [i32, i32, i32, i32]),      # an answer (0 or 1), not a status
    "mp_gmm_aggregate_bins_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, i64, i32, c_p, c_p, i32, c_p, i64, i32, c_p,
                                        c_p, i64, c_p]),
    "mp_gmm_aggregate_gather_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, i64, i32, c_p, c_p, i32, c_p, i64, i32,
                                          c_p, c_p, c_p, i64, c_p]),
    "mp_gmm_grad_chunk": (i64, [i64, i32, i32]),   # an answer (edges per chunk), or -MP_ERR_ARG
    "mp_gmm_param_grad_workspace": (sz, [i64, i32, i32]),
    "mp_gmm_param_grad_f32": (i64, [c_p, c_p, i64, c_p, i64, i32, c_p, c_p, i32, c_p, i64, c_p, i64, i32, c_p, c_p,
                                    c_p, i64, c_p, sz, c_p]),
    # the attention readout (csrc/mp_glob.hip): int64 returns again, the sign tested by ops._count_call
    "mp_readout_path": (i64, [i64, i32]),          # an answer (0, 1 or 2), or -MP_ERR_ARG
    "mp_readout_chunk": (i64, [i32]),              # nodes per chunk of a split graph, or -MP_ERR_ARG
    "mp_readout_workspace": (sz, [i64, i64, i64, i32]),
    "mp_attention_readout_f32": (i64, [c_p, i64, i64, i32, c_p, i64, i64, c_p, i64, c_p, c_p, i64, sz, c_p, sz, c_p,
                                       sz, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_attention_readout_bwd_f32": (i64, [c_p, i64, c_p, i64, i64, i32, c_p, i64, i64, c_p, i64, c_p, c_p, c_p, i64,
                                           c_p, i64, sz, c_p, i64, sz, c_p, sz, c_p, sz, c_p]),
    # RGCNConv (csrc/mp_rgcn.hip): int64 returns again, the sign tested by ops._count_call
    "mp_rgcn_ok": (i64, [i32, i32, i32, i32]),     # an answer (0 or 1), not a status
    "mp_rgcn_att_chunk": (i64, []),                # edges per stage-1 workgroup of the att gradient
    "mp_rgcn_aggregate_bins_f32": (i64, [ctypes.POINTER(MpCsr), c_p, c_p, i64, c_p, i64, sz, i32, i32, c_p, i64, i32,
                                         c_p, i64, i64, sz, c_p]),
    "mp_rgcn_aggregate_gather_f32": (i64, [ctypes.POINTER(MpCsr), c_p, c_p, i64, c_p, i64, sz, i32, i32, c_p, i64, i64,
                                           sz, i32, c_p, c_p, i64, c_p]),
    "mp_rgcn_att_grad_workspace": (sz, [i64, i32, i32]),
    "mp_rgcn_att_grad_f32": (i64, [c_p, c_p, c_p, c_p, i64, c_p, c_p, i64, i64, c_p, i64, i32, i32, i32, c_p, i64, sz,
                                   c_p, sz, c_p]),
    # DNAConv (csrc/mp_dna.hip): int64 returns again, the sign tested by ops._count_call
    "mp_dna_ok": (i64, [i32, i32, i32]),           # an answer (0 or 1), not a status
    "mp_dna_max_layers": (i64, [i32, i32]),        # the largest fused T of an (H, C) pair, 0 = none
    "mp_dna_split_chunk": (i64, []),               # the schedule's task size from which the kernels walk tasks
    "mp_dna_workspace": (sz, [ctypes.POINTER(MpCsr), i64]),
    "mp_dna_aggregate_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, sz, c_p, i64, sz, c_p, i64, sz, c_p, i64, i32, i32,
                                   i32, u64, f32, c_p, i64, sz, c_p, sz, c_p, sz, c_p]),
    "mp_dna_backward_dst_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, sz, c_p, i64, sz, c_p, i64, sz, c_p, i64, c_p,
                                      i64, sz, c_p, sz, i32, i32, i32, u64, f32, c_p, i64, sz, c_p, sz, c_p]),
    "mp_dna_backward_src_f32": (i64, [ctypes.POINTER(MpCsr), c_p, i64, sz, c_p, i64, sz, c_p, i64, sz, c_p, i64, c_p,
                                      i64, sz, c_p, sz, i32, i32, i32, u64, f32, c_p, i64, sz, c_p, i64, sz, c_p, sz,
                                      c_p]),
    "mp_dna_dropout_keep": (i64, [u64, f32, i32, i32, i64, c_p, sz, c_p]),
    # the dense family (csrc/mp_dense.hip): int64 returns again, the sign tested by ops._count_call
    "mp_diff_pool_path": (i64, [i64, i32, i32]),   # an answer (0 or 1), or -MP_ERR_ARG
    "mp_diff_pool_workspace": (sz, [i64, i64, i32, i32]),
    "mp_diff_pool_bwd_workspace": (sz, [i64, i64, i32, i32]),
    "mp_dense_diff_pool_f32": (i64, [c_p, c_p, c_p, c_p, i64, i64, i32, i32, c_p, sz, c_p, sz, c_p, sz, c_p, sz, c_p,
                                     sz, c_p, sz, c_p, sz, c_p]),
    "mp_dense_diff_pool_bwd_f32": (i64, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, i64, i64, i32, i32, c_p, sz, c_p, sz,
                                         c_p, sz, c_p]),
    "mp_dense_mean_agg_f32": (i64, [c_p, c_p, i64, i64, i32, i32, i32, c_p, c_p, sz, c_p, sz, c_p]),
    "mp_to_dense_batch_f32": (i64, [c_p, i64, i32, c_p, i64, i64, f32, c_p, sz, c_p, sz, c_p]),
    "mp_to_dense_batch_bwd_f32": (i64, [c_p, i64, i32, c_p, i64, i64, c_p, sz, c_p]),
    "mp_to_dense_adj_workspace": (sz, [i64, i64, i32]),
    "mp_to_dense_adj_f32": (i64, [c_p, c_p, i64, c_p, i32, c_p, i64, c_p, i64, i64, c_p, sz, c_p, sz, c_p]),
    # link prediction (csrc/mp_link.hip): int64 returns again, the sign tested by ops._count_call
    "mp_link_lanes": (i64, [i32, i32]),            # lanes per edge of a width, or -MP_ERR_ARG
    "mp_edge_score_f32": (i64, [c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, c_p, sz, c_p]),
    "mp_link_loss_workspace": (sz, [i64]),
    "mp_link_loss_f32": (i64, [c_p, c_p, i64, c_p, i64, i64, i32, i32, i32, c_p, sz, c_p, sz, c_p, sz, c_p]),
    "mp_link_grad_rows_f32": (i64, [c_p, c_p, c_p, i64, i64, c_p, i64, c_p, i64, i64, i32, i32, c_p, i64, sz, c_p]),
    "mp_neg_sample": (i64, [c_p, sz, c_p, i64, i32, u64, i64, c_p, c_p, sz, c_p]),
    "mp_neg_sample_rows": (i64, [c_p, sz, c_p, i64, u64, c_p, i64, c_p, sz, c_p]),
}
MP_NEG_FULL = 0
MP_NEG_UPPER = 1

# Of the symbols declared `int` / `int32_t`, these answer a question (a version,
# a count, a yes / no); every other one returns a status: MP_OK, or a code with
# the reason in mp_last_error().  (ctypes.c_int32 is ctypes.c_int, so the types
# cannot tell the two kinds apart.)
VALUE_RETURNING = ("mp_abi_version", "mp_schedule_n_waves", "mp_gat_train_ok", "mp_gat_two_pass_ok",
                   "mp_gat_wide_ok", "mp_gat_bwd_blocks", "mp_arg_mask_words", "mp_spline_ok", "mp_topk_path",
                   "mp_pool_score_bwd_parts", "mp_cluster_max_blocks")
STATUS_RETURNING = tuple(name for name, (res, _) in SIGNATURES.items()
                         if res is ctypes.c_int and name not in VALUE_RETURNING)

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


class NativeLibraryStale(RuntimeError):
    pass


# the C-ABI version these bindings are written for (include/mi355_mp.h MP_ABI_VERSION)
ABI_VERSION = 7


def load(path=None):
    """Load (once) and return the native library; raise if it is absent, or
    (the in-tree library) if it was built from other sources than the ones
    beside it -- the library carries its source hash (mp_source_hash)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NativeLibraryMissing(
            "mi355_mp: native library %s not found; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % p)
    if path is None and os.path.abspath(p) == os.path.abspath(DEFAULT_LIB_PATH):
        built = library_hash(p)
        want = source_hash()
        if built != want:
            raise NativeLibraryStale(
                "mi355_mp: %s was built from sources %s, the tree holds %s; rebuild it with "
                "`python -c 'import __graft_entry__ as g; g.build()'`" % (p, built, want))
    # RTLD_LOCAL: every build keeps its own kernels.  With RTLD_GLOBAL a second build
    # loaded into the process (an A/B variant) binds its template kernel stubs to the
    # first build's same-named definitions and silently runs the first build's code.
    lib = ctypes.CDLL(p, mode=ctypes.RTLD_LOCAL)

    def raise_on_status(rc, func, args):
        if rc != MP_OK:
            check(rc, func.__name__, lib)   # the text comes from the library that refused
        return rc

    lib.raising = types.SimpleNamespace()   # the view native() returns
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
        if name in STATUS_RETURNING:
            # item access makes a function object of its own, so the errcheck set on it
            # leaves lib.<name> (attribute access, cached) returning the code
            fn = lib[name]
            fn.restype, fn.argtypes, fn.errcheck = res, args, raise_on_status
        setattr(lib.raising, name, fn)
    if lib.mp_abi_version() != ABI_VERSION:
        raise NativeLibraryStale("mi355_mp: %s has C-ABI %d, these bindings need %d" % (p, lib.mp_abi_version(),
                                                                                       ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


def native(path=None):
    """The library load(path) returns, as a view whose status-returning
    functions (STATUS_RETURNING) raise RuntimeError "<symbol> failed (code
    <rc>): <mp_last_error() text>" on a nonzero status instead of returning it;
    size queries, *_ok, counts and strings are load()'s plain functions.  The
    package calls the library through this view, so a call the library rejects
    (before any launch) cannot go unnoticed."""
    return load(path).raising


def library_hash(path=None):
    """The source hash compiled into a library file (mp_source_hash); needs no
    GPU.  'unknown' for a library built without it."""
    lib = ctypes.CDLL(path or LIB_PATH, mode=ctypes.RTLD_LOCAL)
    try:
        fn = lib.mp_source_hash
    except AttributeError:
        return "unknown"
    fn.restype = ctypes.c_char_p
    fn.argtypes = []
    return fn().decode()


def source_hash():
    """sha256 over the native sources the library is built from (csrc/*.hip,
    csrc/*.h, csrc/*.cpp, csrc/Makefile, include/mi355_mp.h); the Makefile
    compiles the same hash into the library.  Profile summaries record it, so a
    committed counter profile is only used for the build it measured."""
    import glob
    import hashlib
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))
                   + glob.glob(os.path.join(csrc, "*.cpp")))
    files += [os.path.join(csrc, "Makefile"),
              os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "mi355_mp.h")]
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def kernel_name(csr_struct, w, x, ldx, F, reduce, bias, out, ldo, device=None):
    """Demangled name of the main kernel mp_aggregate_f32 dispatches for these
    arguments (mp_aggregate_kernel_name)."""
    buf = ctypes.create_string_buffer(1024)
    native().mp_aggregate_kernel_name(csr_struct, w, x, ldx, F, MP_REDUCE[reduce], bias, out, ldo, buf, 1024,
                                      stream_ptr(device))
    return buf.value.decode()


def check(rc, what, lib=None):
    if rc != MP_OK:
        msg = (lib or load()).mp_last_error().decode(errors="replace")
        raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg))


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def nbytes(t):
    """Extent in bytes of a caller-allocated array passed to the C-ABI (ABI 6:
    workspaces and partial arrays travel with their size; 0 for None)."""
    return 0 if t is None else t.numel() * t.element_size()


def require_device(*tensors):
    """Every hot-path op runs on the GPU only; there is no CPU fallback."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mi355_mp: tensors must be on a ROCm (cuda) device; got %s. "
                "The MI355X engine has no CPU fallback." % t.device)
