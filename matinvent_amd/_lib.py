"""ctypes binding of include/matinvent_hip.h.  No fallback: if the HIP library is missing or
a call fails, this raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI_LIB_PATH") or os.path.join(HERE, "lib", "libmatinvent_hip.so")   # (MI_LIB_PATH: an A/B build of scripts/build_variant.py)

NCOEF = 16
NUM_TYPES = 100


class NetConfig(C.Structure):
    _fields_ = [("hidden_dim", C.c_int), ("num_layers", C.c_int), ("num_freqs", C.c_int), ("time_dim", C.c_int),
                ("ln", C.c_int)]


class SamplerNoise(C.Structure):
    _fields_ = [("corr_x", C.c_void_p), ("pred_l", C.c_void_p), ("pred_t", C.c_void_p), ("pred_x", C.c_void_p)]


class SamplerRecord(C.Structure):
    _fields_ = [("atom_types", C.c_void_p), ("frac_coords", C.c_void_p), ("lattices", C.c_void_p),
                ("frac_coords_mid", C.c_void_p), ("log_prob_l", C.c_void_p), ("log_prob_t", C.c_void_p),
                ("log_prob_x", C.c_void_p)]


class GemNetConfig(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("emb_atom", "emb_edge", "emb_trip", "emb_rbf", "emb_cbf", "emb_bil", "num_radial", "num_spherical",
                                       "num_blocks", "num_before_skip", "num_after_skip", "num_concat", "num_atom", "max_neighbors",
                                       "max_images")] + [("cutoff", C.c_float)]


class MGCorruption(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("sigma_min", "sigma_max", "beta_min", "beta_max", "limit_density", "limit_var_scale")] + [("d3pm_steps", C.c_int)]


class MGSamplerNoise(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("corr_pos", "corr_cell", "pred_pos", "pred_cell", "pred_u1", "pred_u2")]


_P, _I, _L, _U64, _U32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32

# name -> (restype, argtypes); mirrors include/matinvent_hip.h one to one
SIGNATURES = {
    "mi_last_error": (C.c_char_p, []),
    "mi_version": (_I, []),
    "mi_trace_push": (_I, [C.c_char_p]),
    "mi_trace_pop": (_I, []),
    "mi_net_create": (_I, [C.POINTER(NetConfig), C.POINTER(_P)]),
    "mi_net_destroy": (None, [_P]),
    "mi_net_num_params": (_L, [_P]),
    "mi_net_num_tensors": (_I, [_P]),
    "mi_net_param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I), C.POINTER(_I)]),
    "mi_net_set_params": (_I, [_P, _P, C.POINTER(C.c_float), _P]),
    "mi_batch_create": (_I, [_P, C.POINTER(_I), _I, _L, _L, C.POINTER(_P)]),
    "mi_batch_create_knn": (_I, [_P, C.POINTER(_I), _I, _L, _L, _I, _I, C.POINTER(_P)]),
    "mi_knn_graph": (_I, [_P, _P, _P, _P, C.POINTER(_L)]),
    "mi_knn_graph_read": (_I, [_P, _P, _P, _I, _P]),
    "mi_structure_check": (_I, [_P, _P, _P, _P, _P]),
    "mi_structure_check_offsets": (_I, [_P, _I, _P, _P, _P, _P]),
    "mi_debug_spin": (_I, [C.c_longlong, _P]),
    "mi_set_edge_pairs": (_I, [_I]),
    "mi_set_concurrent_groups": (_I, [_I]),
    "mi_knn_graph_status": (_I, [_P, _P]),
    "mi_plane_format": (_I, []),
    "mi_terms_per_product": (_I, []),
    "mi_debug_mfma_flops": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), _I]),
    "mi_debug_fourier_pairs": (_I, [_P, _P, _P, _L, _I, _P, _P]),
    "mi_debug_set_db_min_tiles": (_I, [_I]),
    "mi_debug_set_node_planes_min_rows": (_I, [_I]),
    "mi_debug_set_tn128": (_I, [_I]),
    "mi_debug_set_tn_split_min_rows": (_I, [_I]),
    "mi_debug_set_tn_target_tiles": (_I, [_I]),
    "mi_debug_set_pair_wide": (_I, [_I]),
    "mi_debug_set_planes_small_tiles": (_I, [_I]),
    "mi_debug_set_planes_big": (_I, [_I, _I]),
    "mi_debug_set_planes_rt": (_I, [_I, _I]),
    "mi_debug_set_planes_latency": (_I, [_I]),
    "mi_debug_set_planes_dma": (_I, [_I]),
    "mi_debug_set_planes_big_seg": (_I, [_I]),
    "mi_debug_set_node_priority": (_I, [_I]),
    "mi_debug_set_node_fused": (_I, [_I]),
    "mi_debug_node_chain_clock": (_I, [_P]),
    "mi_debug_set_edge2_fused": (_I, [_I]),
    "mi_debug_set_node_train": (_I, [_I]),
    "mi_debug_set_node_bwd": (_I, [_I, _I]),
    "mi_debug_set_knn_nosync": (_I, [_I]),
    "mi_debug_set_node_split": (_I, [_I]),
    "mi_debug_set_node_cols": (_I, [_I]),
    "mi_debug_set_node_touch": (_I, [_I]),
    "mi_debug_set_heads_rows16": (_I, [_I]),
    "mi_debug_set_eval_reuse": (_I, [_I]),
    "mi_debug_set_skip": (_I, [_I]),
    "mi_debug_rt_clock": (_I, [_P, _I, _I]),
    "mi_debug_set_rt_lean": (_I, [_I]),
    "mi_debug_set_edge_fused": (_I, [_I]),
    "mi_debug_edge2_clock": (_I, [_P]),
    "mi_debug_set_edge1_fused": (_I, [_I]),
    "mi_debug_edge1_clock": (_I, [_P]),
    "mi_batch_destroy": (None, [_P]),
    "mi_batch_num_nodes": (_I, [_P]),
    "mi_batch_num_edges": (_L, [_P]),
    "mi_batch_node2graph": (_P, [_P]),
    "mi_cspnet_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_cspnet_tap": (_I, [_P, _P, _I, _P, _P]),
    "mi_time_embedding": (_I, [_P, _P, _I, _I, _P, _P]),
    "mi_sampler_init_state": (_I, [_P, _U64, _I, _P, _P, _P, _P]),
    "mi_sampler_run": (_I, [_P, _P, C.POINTER(C.c_float), _I, _I, _I, _P, _U64, C.POINTER(SamplerNoise),
                            C.POINTER(SamplerRecord), _P, _P, _P, _P]),
    "mi_philox_fill": (_I, [_U64, _U32, _U32, _L, _L, _I, _P, _P]),
    "mi_cspnet_forward_train": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_cspnet_backward": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "mi_batch_set_wgrad_window": (_I, [_P, _P, _I]),
    "mi_cspnet_wgrad_flush": (_I, [_P, _P, _P, _P]),
    "mi_batch_wgrad_pending": (_I, [_P]),
    "mi_adam_step": (_I, [_P, _P, _P, _P, _L, _I, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "mi_add_noise": (_I, [_P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _U64, _U32, _P, _P, _P, _P, _P, _P, _P,
                          _P, _P, _P]),
    "mi_add_noise_per_crystal": (_I, [_P, _P, _P, _P, _P, _P, _U64, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_sampler_set_keep": (_I, [_P, _I, _I]),
    "mi_ft_micro_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, C.c_float, C.c_float, C.c_float, C.c_float, _U64, _U32, _P, _P, _P,
                              C.c_float, C.c_float, C.c_float, C.c_float, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mi_ft_micro_steps_stacked": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _U64, _U32, _P, _P, _P,
                                       C.c_float, C.c_float, C.c_float, C.c_float, _I, _I, _P, _P, _P, _P]),
    "mi_gemnet_create": (_I, [C.POINTER(GemNetConfig), C.POINTER(_P)]),
    "mi_gemnet_destroy": (None, [_P]),
    "mi_gemnet_num_params": (_L, [_P]),
    "mi_gemnet_num_tensors": (_I, [_P]),
    "mi_gemnet_param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I), C.POINTER(_I)]),
    "mi_gemnet_set_params": (_I, [_P, _P, _P]),
    "mi_gbatch_create": (_I, [_P, C.POINTER(_I), _I, _L, _L, C.POINTER(_P)]),
    "mi_gbatch_destroy": (None, [_P]),
    "mi_gbatch_set_offsets": (_I, [_P, _L, _L]),
    "mi_gemnet_graph": (_I, [_P, _P, _P, _P, _P, C.POINTER(_L)]),
    "mi_gemnet_graph_read": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_gemnet_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mi_gemnet_backward": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "mi_debug_set_mg_f16": (_I, [_I]),
    "mi_debug_set_mg_planes": (_I, [_I]),
    "mi_debug_set_mg_lean": (_I, [_I]),
    "mi_debug_set_mg_nosync": (_I, [_I]),
    "mi_debug_set_mg_deg_cap": (_I, [_I]),
    "mi_gbatch_graph_status": (_I, [_P, _P, C.POINTER(_I), _P]),
    "mi_gemnet_tap": (_I, [_P, C.c_char_p, _P, _L, C.POINTER(_L), _P]),
    "mi_mg_sample_marginal": (_I, [_P, C.POINTER(MGCorruption), _P, _P, _P, _P, _U64, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_mg_sampler_init": (_I, [_P, C.POINTER(MGCorruption), _U64, _P, _P, _P, _P, _P, _P]),
    "mi_mg_sampler_run": (_I, [_P, _P, C.POINTER(MGCorruption), _I, _I, _I, C.POINTER(C.c_float), _U64, C.POINTER(MGSamplerNoise), _P, _P, _P,
                               _P, _P, _P]),
    "mi_set_gemm_mode": (_I, [_I]),
    "mi_net_set_edge_mode": (_I, [_P, _I]),
    "mi_debug_gemm": (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    "mi_saturation_events": (_I, [C.POINTER(_L), _I]),
    "mi_profile_enable": (_I, [_P, _I]),
    "mi_profile_read": (_I, [_P, C.POINTER(_L), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

# the trajectory extension, include/matinvent_hip_traj.h (a header of its own: SIGNATURES above is the boundary header + the debug header)
TRAJ_SIGNATURES = {
    "mi_traj_logprob": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "mi_traj_logprob_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

# the policy-gradient extension, include/matinvent_hip_pg.h (a header of its own: TRAJ_SIGNATURES above is the trajectory header)
PG_SIGNATURES = {
    "mi_traj_pg_step": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_float, _P, _P, _P, _P]),
}

# the KL-anchored policy-gradient extension, include/matinvent_hip_pg_kl.h (a header of its own: PG_SIGNATURES above is the policy-gradient header)
PG_KL_SIGNATURES = {
    "mi_traj_pg_kl_step": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, C.c_float, C.c_float, _P, _P,
                                _P, _P, _P, _P]),
}

# the optimizer extension, include/matinvent_hip_optim.h (gradient-norm clipping and the non-finite-step guard of the fused Adam)
OPTIM_SIGNATURES = {
    "mi_optim_state_bytes": (_L, []),
    "mi_optim_workspace_bytes": (_L, [_L]),
    "mi_optim_sweep_elems": (_L, [_L]),
    "mi_grad_norm": (_I, [_P, _L, C.c_float, C.c_float, _I, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    "mi_adam_step_guarded": (_I, [_P, _P, _P, _P, _L, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P]),
}

# the strided-chain extension, include/matinvent_hip_stride.h (a batch handle's step-index -> trained-time map)
STRIDE_SIGNATURES = {
    "mi_batch_set_time_map": (_I, [_P, C.POINTER(_I), _I]),
}

# the conditioning extension, include/matinvent_hip_cond.h (replacement conditioning of the reverse chain: a batch handle's known part)
class Condition(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("known_types_host", "known_coords_host", "known_lattice_host", "types0_host", "frac0_host", "lat0_host")]


COND_SIGNATURES = {
    "mi_batch_set_condition": (_I, [_P, C.POINTER(Condition), C.POINTER(C.c_float), _I]),
    "mi_condition_apply": (_I, [_P, _I, _U64, _P, _P, _P, _P]),
}

# the likelihood-mask extension, include/matinvent_hip_lik.h (the trajectory likelihood of a conditioned chain: which predictor terms leave it)
LIK_SIGNATURES = {
    "mi_batch_set_likelihood_mask": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "mi_batch_has_likelihood_mask": (_I, [_P]),
    "mi_traj_read_derivatives": (_I, [_P, _P, _P, _P, _P]),
}

# the structure-fingerprint extension, include/matinvent_hip_fp.h (the key of the structure-resolved long-term memory and replay buffer)
class FpParams(C.Structure):
    _fields_ = [("r_max", C.c_float), ("sigma", C.c_float), ("nbins", C.c_int)]


FP_MAX_SPECIES, FP_MAX_BLOCKS, FP_MAX_BINS, FP_MAX_REACH, FP_CUT = 8, 36, 64, 16, 6.0   # include/matinvent_hip_fp.h
FP_OK, FP_SPECIES, FP_NONFINITE, FP_VOLUME, FP_REACH, FP_ATOMS = 0, 1, 2, 3, 4, 5

FP_SIGNATURES = {
    "mi_structure_fingerprint_offsets": (_I, [_P, _I, _P, _P, _P, C.POINTER(FpParams), _P, _P, _P]),
    "mi_structure_fingerprint": (_I, [_P, _P, _P, _P, C.POINTER(FpParams), _P, _P, _P]),
}

# the preference extension, include/matinvent_hip_dpo.h (a batch handle's ranked pairs and the Diffusion-DPO micro-step)
DPO_SIGNATURES = {
    "mi_batch_set_pairs": (_I, [_P, C.POINTER(_I), C.POINTER(_I), _I]),
    "mi_batch_num_pairs": (_I, [_P]),
    "mi_dpo_micro_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, C.c_float, C.c_float, C.c_float, C.c_float, _U64, _U32, _P, _P, _P,
                               C.c_float, C.c_float, C.c_float, C.c_float, _I, _I, _P, _P, _P, _P, _P, _P]),
}

# the fingerprint-matching extension, include/matinvent_hip_match.h (nearest bank row, count within a tolerance, pair distances)
class FpMatchArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("query", "bank", "bank_start", "bank_len", "grp_q_off", "q_idx", "grp_c_off", "c_idx", "grp_ncols", "items",
                                           "grp_part_off", "workspace", "best_dist", "best_idx", "n_within", "status", "pair_dist", "pair_off")] +
                [("bank_floats", C.c_int64), ("pair_floats", C.c_int64)] +
                [(k, C.c_int) for k in ("Q", "row_stride", "M", "G", "nnz_q", "nnz_c", "n_items", "n_partials", "max_ncols")] + [("tol", C.c_float)])


FP_MATCH_TILE, FP_MATCH_ITEM_INTS = 8, 5   # include/matinvent_hip_match.h

MATCH_SIGNATURES = {
    "mi_fp_match_plan": (_I, [C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_L), C.POINTER(_L)]),
    "mi_fp_match_workspace": (_L, [_L]),
    "mi_fp_match": (_I, [C.POINTER(FpMatchArgs), _P]),
}

# the resampling extension, include/matinvent_hip_resample.h (RePaint's jumps for the conditioned chain: a batch handle's (r, j) and jump table)
RESAMPLE_SIGNATURES = {
    "mi_batch_set_resampling": (_I, [_P, C.POINTER(C.c_float), _I, _I, _I]),
    "mi_resample_jump": (_I, [_P, _I, _U64, _P, _P, _P, _P]),
    "mi_resample_schedule": (_L, [_I, _I, _I, C.POINTER(_I), _L]),
    "mi_resample_visit_seed": (_U64, [_U64, _U32]),
}

# the supervised-training extension, include/matinvent_hip_pretrain.h (one denoising-training micro-step of one network)
PRETRAIN_SIGNATURES = {
    "mi_pretrain_micro_step": (_I, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), _P, _P, _I, _U64, _U32, _P, _P, _P, C.c_float, C.c_float, C.c_float,
                                    _I, _I, _I, _P, _P, _P, _P]),
}

# the handle-pool extension, include/matinvent_hip_pool.h (a device-memory pool for batch handles and the pooled handle)
POOL_SIGNATURES = {
    "mi_pool_create": (_I, [_P, _L, C.POINTER(_P)]),
    "mi_pool_destroy": (_I, [_P]),
    "mi_pool_trim": (_I, [_P]),
    "mi_pool_stats": (_I, [_P, C.POINTER(_L)]),
    "mi_pool_block_bytes": (_L, [_L]),
    "mi_pool_set_poison": (_I, [_P, _I]),
    "mi_batch_create_pooled": (_I, [_P, _P, C.POINTER(_I), _I, _L, _L, C.POINTER(_P)]),
    "mi_batch_index_table": (_L, [_P, _I, C.POINTER(_I), _L]),
}

# the weight-average extension, include/matinvent_hip_ema.h (the fused Adam step with an exponential moving average of the weights)
EMA_SIGNATURES = {
    "mi_adam_step_ema": (_I, [_P, _P, _P, _P, _P, _L, _I, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _I, _P, _P]),
}

# the guidance extension, include/matinvent_hip_guidance.h (the property-conditioned embedding, its training micro-step, the guided step)
GUIDANCE_MAX_FREQS, GUIDANCE_CLAMP = 12, 8.0   # include/matinvent_hip_guidance.h

GUIDANCE_SIGNATURES = {
    "mi_net_set_latent": (_I, [_P, _I, _I]),
    "mi_net_latent_dim": (_I, [_P]),
    "mi_crystal_embedding": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mi_guidance_drop_mask": (_I, [_U64, _U32, _L, _I, C.c_float, _P, _P]),
    "mi_pretrain_micro_step_cond": (_I, PRETRAIN_SIGNATURES["mi_pretrain_micro_step"][1][:-1] + [_P, _P, _P, C.c_float, _P]),
    "mi_batch_set_guidance": (_I, [_P, _P, C.POINTER(C.c_float), C.POINTER(_I), _I, _I, C.c_float]),
    "mi_batch_clear_guidance": (_I, [_P]),
    "mi_guidance_combine": (_I, [_P, _P, C.c_float, _L, _L, _L, _P, _P]),
}

# the property-predictor extension, include/matinvent_hip_scalar.h (the trunk with a scalar head: inference forward, training micro-step)
SCALAR_LOSS_MSE, SCALAR_LOSS_L1 = 0, 1   # include/matinvent_hip_scalar.h

SCALAR_SIGNATURES = {
    "mi_scalar_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "mi_scalar_micro_step": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, C.POINTER(_I), _P, C.POINTER(_I), _I, _I, _P, _P, _P, _P, _P, _P]),
    "mi_scalar_read": (_I, [_P, _I, _P, _P, _P]),
}

# the steering extension, include/matinvent_hip_steer.h (the noise-aware predictor's two entries and the particle resampling)
STEER_MODE_MAX, STEER_MODE_MIN, STEER_MODE_TARGET = 0, 1, 2   # include/matinvent_hip_steer.h
STEER_MAX_PARTICLES, STEER_DRAW, STEER_NSTATS = 256, 29, 3

STEER_SIGNATURES = {
    "mi_scalar_micro_step_noised": (_I, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), _P, _P, _I, _U64, _U32, _P, _P, _P, _P, _P, _I, _P, _P, C.POINTER(_I),
                                         _P, C.POINTER(_I), _I, _I, _P, _P, _P, _P, _P, _P]),
    "mi_scalar_forward_state": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P]),
    "mi_steer_resample": (_I, [_P, _I, _P, _I, _I, _I, C.c_float, C.c_float, C.c_float, _U64, _U32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

# the classifier-guidance extension, include/matinvent_hip_inputgrad.h (the predictor's input gradient, the seed and the guided shift)
GUIDE_MODE_MAX, GUIDE_MODE_MIN, GUIDE_MODE_TARGET = 0, 1, 2   # include/matinvent_hip_inputgrad.h

INPUT_GRAD_SIGNATURES = {
    "mi_scalar_input_grad": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "mi_guide_seed": (_I, [_P, _I, _I, _I, _I, C.c_float, _P, _P]),
    "mi_guide_shift": (_I, [_P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
}

# the relaxation extension, include/matinvent_hip_relax.h (FIRE on the forces of the predictor read as an energy)
RELAX_ACTIVE, RELAX_CONVERGED, RELAX_FAILED, RELAX_EXHAUSTED = 0, 1, 2, 3   # include/matinvent_hip_relax.h
RELAX_NF, RELAX_NI, RELAX_MAX_ROWS = 6, 3, 1500


class RelaxParams(C.Structure):
    _fields_ = ([(k, C.c_float) for k in ("dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a", "fmax", "scale", "cell_factor", "det_min")] +
                [(k, C.c_int) for k in ("n_min", "relax_cell", "per_atom")])


RELAX_SIGNATURES = {
    "mi_relax_init": (_I, [_P, C.POINTER(RelaxParams), _I, _I, _P, _P, _P, _P, _P, _P]),
    "mi_relax_step": (_I, [_P, C.POINTER(RelaxParams), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mi_relax_run": (_I, [_P, _P, C.POINTER(RelaxParams), _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
}

# the convex-hull extension, include/matinvent_hip_hull.h (energy above the lower hull of a bank of reference phases)
HULL_MAX_ELEMS, HULL_MAX_ITERS, HULL_EPS, HULL_LDS_DOUBLES = 8, 256, 1e-12, 4096   # include/matinvent_hip_hull.h
HULL_OK, HULL_NO_TERMINAL, HULL_UNBOUNDED, HULL_ITER_CAP, HULL_BAD_QUERY = 0, 1, 2, 3, 4
HULL_FLAG_SKIPPED = 1


class HullArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("bank_nelem", "bank_Z", "bank_frac", "bank_energy", "grp_nelem", "grp_Z", "grp_q_off", "q_idx", "grp_c_off", "c_idx",
                                           "query_c", "query_e", "workspace", "e_hull", "e_above", "chempot", "decomp_frac", "decomp_idx", "iters", "status",
                                           "flags")] +
                [(k, C.c_int) for k in ("M", "G", "Q", "nnz_q", "nnz_c", "max_elems", "no_lds")])


HULL_SIGNATURES = {
    "mi_hull_workspace": (_L, [_I, _I, _I]),
    "mi_hull_above": (_I, [C.POINTER(HullArgs), _P]),
}

# the vibration extension, include/matinvent_hip_vib.h (Gamma-point modes and harmonic thermodynamics of the predictor read as an energy)
VIB_OK, VIB_NO_CONVERGENCE, VIB_BAD_INPUT = 0, 1, 2   # include/matinvent_hip_vib.h
VIB_MAX_ATOMS, VIB_MAX_TEMPS, EIG_MAX_SWEEPS, EIG_LDS_MAX_M, EIG_MAX_M = 256, 8, 30, 128, 768


class VibChunkArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("src_types", "src_frac", "src_lat", "src_node_off")] + [("Bs", C.c_int)] +
                [(k, C.c_void_p) for k in ("plan_src", "plan_copy", "types", "frac", "lat", "g_frac", "workspace", "ws_off")] +
                [(k, C.c_double) for k in ("h", "scale", "det_min")] + [("per_atom", C.c_int)])


class VibDynmatArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("workspace", "ws_off", "node_off", "mass", "asym", "status")] + [("h", C.c_double), ("B", C.c_int), ("max_atoms", C.c_int)])


class SymEigArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("mats", "mat_off", "sizes", "work", "work_off", "evals", "ev_off", "sweeps", "status")] +
                [(k, C.c_int) for k in ("B", "max_size", "no_lds")])


class VibThermoArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("evals", "ev_off", "sizes", "eig_status", "dyn_status", "freqs", "c_v", "zpe", "n_imag", "n_zero", "status")] +
                [("temps", C.c_double * 8), ("nu_cut", C.c_double), ("B", C.c_int), ("K", C.c_int)])


VIB_SIGNATURES = {
    "mi_vib_workspace": (_L, [C.POINTER(_I), _I, C.POINTER(_L)]),
    "mi_vib_displace": (_I, [_P, C.POINTER(VibChunkArgs), _P]),
    "mi_vib_collect": (_I, [_P, C.POINTER(VibChunkArgs), _P]),
    "mi_vib_run_chunk": (_I, [_P, _P, C.POINTER(VibChunkArgs), _P, _P, _P, _I, _P, _P, _P, _P]),
    "mi_vib_dynmat": (_I, [C.POINTER(VibDynmatArgs), _P]),
    "mi_sym_eigvals": (_I, [C.POINTER(SymEigArgs), _P]),
    "mi_vib_thermo": (_I, [C.POINTER(VibThermoArgs), _P]),
}

# the phonon extension, include/matinvent_hip_phonon.h (force constants from home-cell displacements in a supercell, dynamical matrices on a q-mesh)
PHONON_MAX_PRIM, PHONON_IMAGES = 128, 27   # include/matinvent_hip_phonon.h


class PhononFcArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("workspace", "ws_off", "node_off", "mass", "frac", "lat", "asym", "status")] +
                [(k, C.c_double) for k in ("h", "tie_tol", "det_min")] + [("reps", C.c_int * 3), ("B", C.c_int), ("max_atoms", C.c_int)])


class PhononDynmatArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("workspace", "ws_off", "node_off", "mass", "fc_status", "table", "item_crystal", "item_q", "mats", "mat_off", "sizes",
                                           "herm")] + [("table_len", C.c_int64), ("reps", C.c_int * 3)] + [(k, C.c_int) for k in ("B", "Q", "T")])


class PhononThermoArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("evals", "ev_off", "sizes", "eig_status", "sweeps", "herm_item", "fc_status", "item_off", "item_q", "weight", "lam",
                                           "freqs", "c_v", "zpe", "n_imag", "n_zero", "min_freq", "min_q", "herm", "pair_gap", "sweeps_max", "status")] +
                [("temps", C.c_double * 8), ("nu_cut", C.c_double)] + [(k, C.c_int) for k in ("B", "K", "Q")])


PHONON_SIGNATURES = {
    "mi_phonon_workspace": (_L, [C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_L)]),
    "mi_phonon_fc": (_I, [C.POINTER(PhononFcArgs), _P]),
    "mi_phonon_dynmat": (_I, [C.POINTER(PhononDynmatArgs), _P]),
    "mi_phonon_thermo": (_I, [C.POINTER(PhononThermoArgs), _P]),
}

# the elasticity extension, include/matinvent_hip_elastic.h (the elastic tensor and moduli of the predictor read as an energy)
ELASTIC_OK, ELASTIC_BAD_INPUT, ELASTIC_SINGULAR = 0, 1, 2   # include/matinvent_hip_elastic.h
ELASTIC_COPIES, ELASTIC_ROW = 13, 8


class ElasticChunkArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("src_types", "src_frac", "src_lat", "src_node_off")] + [("Bs", C.c_int)] +
                [(k, C.c_void_p) for k in ("plan_src", "plan_copy", "types", "frac", "lat", "g_frac", "g_lat", "istate", "workspace", "asym")] +
                [(k, C.c_double) for k in ("h", "scale", "det_min")] + [("per_atom", C.c_int)])


class ElasticFitArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("workspace", "C", "S", "stress0", "pressure", "asym", "asym_C", "moduli", "evals", "cond", "n_negative",
                                           "n_unrelaxed", "status")] + [("h", C.c_double), ("B", C.c_int)])


ELASTIC_SIGNATURES = {
    "mi_elastic_strain": (_I, [_P, C.POINTER(ElasticChunkArgs), _P]),
    "mi_elastic_collect": (_I, [_P, C.POINTER(ElasticChunkArgs), _P]),
    "mi_elastic_run_chunk": (_I, [_P, _P, C.POINTER(ElasticChunkArgs), C.POINTER(RelaxParams), _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "mi_elastic_fit": (_I, [C.POINTER(ElasticFitArgs), _P]),
}

# the structure matcher, include/matinvent_hip_smatch.h (lattice maps, species-constrained assignment, RMS distance)
SM_MAX_ATOMS, SM_SMALL_ATOMS, SM_MAX_SPECIES, SM_MAX_MAPS = 64, 32, 16, 256   # include/matinvent_hip_smatch.h
SM_PREP_OK, SM_PREP_BAD_INPUT, SM_PREP_TOO_MANY_ATOMS, SM_PREP_TOO_MANY_SPECIES, SM_PREP_DEGENERATE_CELL, SM_PREP_REDUCE_CAP = 0, 1, 2, 3, 4, 5
SM_OK, SM_NO_LATTICE, SM_BOX_CAP, SM_MAP_CAP, SM_SPECIES_MISMATCH, SM_BAD_PAIR, SM_NOT_PREPARED = 0, 1, 2, 3, 4, 5, 6


class SmPrepared(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("offsets", "lat", "inv", "frac", "types", "perm", "spec_Z", "spec_off", "info")] + [("B", C.c_int), ("N", C.c_int)])


class SmMatchArgs(C.Structure):
    _fields_ = ([("a", SmPrepared), ("b", SmPrepared)] +
                [(k, C.c_void_p) for k in ("pair_q", "pair_c", "rms", "max_dist", "best_map", "best_trans", "n_maps", "n_items", "status", "perm", "maps")] +
                [("ltol", C.c_double), ("cos_tol", C.c_double), ("P", C.c_int), ("large_tile", C.c_int)])


SMATCH_SIGNATURES = {
    "mi_sm_prepare": (_I, [_P, _P, _P, C.POINTER(SmPrepared), _P]),
    "mi_sm_match": (_I, [C.POINTER(SmMatchArgs), _P]),
}

# the symmetry finder, include/matinvent_hip_sym.h (space-group operations, point group, primitive cell of a prepared set)
SYM_MAX_OPS, SYM_MAX_TRANS, SYM_INFO, SYM_CLASSES = 192, 64, 8, 10   # include/matinvent_hip_sym.h
SYM_OK, SYM_NOT_PREPARED, SYM_BOX_CAP, SYM_MAP_CAP, SYM_NO_LATTICE, SYM_AMBIGUOUS, SYM_OPS_CAP, SYM_NOT_A_GROUP, SYM_PRIM_FAIL, SYM_BAD_TOL = 0, 1, 2, 4, 8, 16, 32, 64, 128, 256


class SymOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("info", "rot_hist", "rot", "trans", "dev", "ptrans")]


class SymPrimArgs(C.Structure):
    _fields_ = ([("set", SmPrepared)] +
                [(k, C.c_void_p) for k in ("types", "frac", "lat", "sym_info", "ptrans", "ws_types", "ws_frac", "prim_count", "prim_status", "prim_det",
                                           "prim_offsets", "out_types", "out_frac", "out_lat")])


SYM_SIGNATURES = {
    "mi_sym_find": (_I, [C.POINTER(SmPrepared), _P, C.c_double, C.POINTER(SymOut), _P]),
    "mi_sym_primitive": (_I, [C.POINTER(SymPrimArgs), _P]),
}

# the conventional cell, include/matinvent_hip_sym_conv.h (basis, centring and Bravais lattice of a primitive crystal)
SYM_CONV_FAIL, SYM_CONV_INFO, SYM_CONV_MAX_MULT = 512, 8, 4   # include/matinvent_hip_sym_conv.h


class SymConvArgs(C.Structure):
    _fields_ = ([("set", SmPrepared)] +
                [(k, C.c_void_p) for k in ("types", "frac", "lat", "sym_info", "sym_rot", "ws_adj", "conv_info", "conv_M", "conv_cvec", "conv_count",
                                           "conv_offsets", "out_types", "out_frac", "out_lat")])


SYM_CONV_SIGNATURES = {
    "mi_sym_conventional": (_I, [C.POINTER(SymConvArgs), _P]),
}

# the refined structure, include/matinvent_hip_sym_refine.h (site maps, orbits, positions and cell projected onto the group)
SYM_REFINE_FAIL, SYM_REFINE_INFO, SYM_REFINE_STAT = 1024, 8, 4   # include/matinvent_hip_sym_refine.h


class SymRefineArgs(C.Structure):
    _fields_ = ([("set", SmPrepared)] +
                [(k, C.c_void_p) for k in ("types", "frac", "lat", "sym_info", "sym_rot", "sym_trans", "out_frac", "out_lat", "orbit", "mult", "site_order",
                                           "trans_ref", "refine_info", "refine_stat")])


SYM_REFINE_SIGNATURES = {
    "mi_sym_refine": (_I, [C.POINTER(SymRefineArgs), _P]),
}

# symmetry-constrained sampling, include/matinvent_hip_symc.h (a batch handle's group, orbits and affine maps; the per-step projection)
SYMC_MAX_ATOMS, SYMC_MAX_OPS = 256, 192   # include/matinvent_hip_symc.h


class SymmetryConstraint(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("op_off_host", "rot_host", "distinct_off_host", "distinct_host", "rep_host", "Q_host", "d_host")]


SYMC_SIGNATURES = {
    "mi_batch_set_symmetry": (_I, [_P, C.POINTER(SymmetryConstraint)]),
    "mi_symmetry_apply": (_I, [_P, _P, _P, _P, _P]),
    "mi_symmetry_failures": (_I, [_P, C.POINTER(_I)]),
}

# composition validity, include/matinvent_hip_chem.h (charge neutrality and the Pauling test over a user-supplied element table)
CHEM_MAX_Z, CHEM_MAX_STATES, CHEM_MAX_ELEMS, CHEM_CHUNK, CHEM_MAX_GRID, CHEM_MAX_BATCH, CHEM_DEFAULT_MAX_COMBOS = 118, 32, 8, 65536, 2048, 4096, 10_000_000   # include/matinvent_hip_chem.h
(CHEM_ENUMERATED, CHEM_ELEMENTAL, CHEM_ALLOY, CHEM_BAD_INPUT, CHEM_TOO_MANY_ELEMENTS, CHEM_UNKNOWN_ELEMENT, CHEM_NO_STATES,
 CHEM_TOO_MANY_COMBOS) = range(8)


class ChemArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("present", "n_states", "ox", "eneg_rank", "is_metal", "node_off", "atom_types", "workspace", "valid", "status", "n_elems",
                                           "elems", "counts", "n_combos", "n_neutral", "n_valid", "first", "first_ox", "atom_ox")] +
                [("max_combos", C.c_int64)] + [(k, C.c_int) for k in ("B", "N", "use_pauling_test", "include_alloys")])


CHEM_SIGNATURES = {
    "mi_chem_workspace": (_L, [_I, _L]),
    "mi_chem_validity": (_I, [C.POINTER(ChemArgs), _P]),
}

# the substrate matcher, include/matinvent_hip_zsl.h (Zur-McGill superlattices, minimal coincident interface area)
ZSL_MAX_MULT, ZSL_MAX_MILLER, ZSL_TABLE, ZSL_ROW_D, ZSL_ROW_I = 63, 8, 3276, 10, 20   # include/matinvent_hip_zsl.h
ZSL_OK, ZSL_NO_MATCH, ZSL_MULT_CAP, ZSL_REDUCE_CAP, ZSL_BAD_CELL = 0, 1, 2, 3, 4


class ZslPlanesArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("lat", "hkl", "cell_of")] + [("C", C.c_int), ("P", C.c_int), ("max_area", C.c_double)] +
                [(k, C.c_void_p) for k in ("vec", "area", "mult", "status")])


class ZslSearchArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("f_vec", "f_area", "f_mult", "f_status", "s_area", "s_mult", "s_status", "s_table")] +
                [(k, C.c_int) for k in ("B", "Pf", "Ps", "count")] + [(k, C.c_double) for k in ("max_area_ratio_tol", "max_length_tol", "max_angle_tol")] +
                [(k, C.c_void_p) for k in ("item_d", "item_i", "item_n")])


class ZslReduceArgs(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("item_d", "item_i", "item_n", "sub_off")] + [(k, C.c_int) for k in ("B", "Pf", "Ps", "S", "count")] +
                [(k, C.c_void_p) for k in ("res_d", "res_i", "res_n", "mcia", "mcia_plane", "mcia_status")])


ZSL_SIGNATURES = {
    "mi_zsl_planes": (_I, [C.POINTER(ZslPlanesArgs), _P]),
    "mi_zsl_workspace": (_L, [_I]),
    "mi_zsl_tables": (_I, [_P, _P, _P, _I, _P, _P]),
    "mi_zsl_search": (_I, [C.POINTER(ZslSearchArgs), _P]),
    "mi_zsl_reduce": (_I, [C.POINTER(ZslReduceArgs), _P]),
}

# every extension table: load() binds SIGNATURES plus these (a new extension header adds its table here)
EXTENSION_SIGNATURES = (TRAJ_SIGNATURES, PG_SIGNATURES, PG_KL_SIGNATURES, OPTIM_SIGNATURES, STRIDE_SIGNATURES, COND_SIGNATURES, FP_SIGNATURES,
                        DPO_SIGNATURES, MATCH_SIGNATURES, LIK_SIGNATURES, RESAMPLE_SIGNATURES, POOL_SIGNATURES, EMA_SIGNATURES, GUIDANCE_SIGNATURES,
                        SCALAR_SIGNATURES, STEER_SIGNATURES, INPUT_GRAD_SIGNATURES, RELAX_SIGNATURES, HULL_SIGNATURES, SMATCH_SIGNATURES, SYM_SIGNATURES, SYM_CONV_SIGNATURES, SYM_REFINE_SIGNATURES, SYMC_SIGNATURES, CHEM_SIGNATURES, ZSL_SIGNATURES, PHONON_SIGNATURES, VIB_SIGNATURES, ELASTIC_SIGNATURES,
                        PRETRAIN_SIGNATURES)

_lib = None


def load():
    """Load the shared library (once) and attach the signatures."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: both must share ONE HIP runtime instance (torch bundles its own libamdhip64);
    # device pointers and streams cross this boundary.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"matinvent_amd: HIP library not found at {LIB_PATH}; build it with `python -m matinvent_amd.build` "
            "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for table in (SIGNATURES,) + EXTENSION_SIGNATURES:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


MI_EINVAL, MI_EHIP, MI_ENOMEM, MI_ESTATE, MI_ECAPACITY = -1, -2, -3, -4, -5   # include/matinvent_hip.h


class MIError(RuntimeError):
    """A failed library call; `code` is the C ABI's return value (MI_EINVAL / MI_EHIP / MI_ENOMEM / MI_ESTATE / MI_ECAPACITY)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().mi_last_error().decode(errors="replace")
        raise MIError(rc, f"matinvent_hip {what} failed (code {rc}): {msg}")


def saturation_events(reset: bool = True) -> int:
    """Number of fp32 -> fp16-plane conversions that had to clamp (or met NaN / inf) since the last reset, over every network and
    stream of the current device (mi_saturation_events; synchronises the device)."""
    n = C.c_int64()
    check(load().mi_saturation_events(C.byref(n), 1 if reset else 0), "mi_saturation_events")
    return int(n.value)


def check_saturation(where: str):
    """Raise if any operand left the range of the two-plane fp16 format since the last check: such results are finite but wrong,
    and must never be handed on silently."""
    check_saturation_count(saturation_events(reset=True), where)


def check_saturation_count(n: int, where: str):
    """check_saturation for a count the caller has read (and reset) itself."""
    if n:
        raise FloatingPointError(
            f"{where}: {n} operand conversions saturated the two-plane fp16 format (values beyond 65504 / scale, or NaN / inf "
            "upstream): the results are outside the stated fp32-class tolerance.  Rebuild with MI_EXTRA_FLAGS=-DMI_PLANES_FP16=0 "
            "(three bf16 planes, no range limit) or use --path f32-gemm")
