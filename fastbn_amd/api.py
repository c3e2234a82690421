"""ctypes binding of include/fastbn.h and the reference-shaped Python classes."""
import atexit
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FBN_LIB_PATH: an alternative build of the same library (A/B runs of build-time switches, tools/)
LIB_PATH = os.environ.get("FBN_LIB_PATH") or os.path.join(_HERE, "libfastbn.so")

_vp, _i32, _i64, _dbl, _cstr = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_char_p
_pp = C.POINTER(C.c_void_p)

# name -> argtypes (all functions return int status except fbn_last_error)
_SIGS = {
    "fbn_version": [_vp, _vp],
    "fbn_device_count": [_vp],
    "fbn_network_load_xmlbif": [_cstr, _pp],
    "fbn_network_create": [C.c_int, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_network_node_counts": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_network_create_cpt": [C.c_int, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_network_node_probs": [_vp, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_network_num_nodes": [_vp, _vp],
    "fbn_network_dims": [_vp, _vp],
    "fbn_network_name": [_vp, C.c_int, C.c_char_p, C.c_int],
    "fbn_network_destroy": [_vp],
    "fbn_evidence_load_libsvm": [_cstr, C.c_int, _vp, _vp, _i64, _vp],
    "fbn_dataset_load_csv": [_cstr, _pp],
    "fbn_synth_forward_sample": [_vp, _i64, C.c_uint64, _vp],
    "fbn_synth_evidence": [_vp, _i64, C.c_int, C.c_uint64, C.c_int, _vp],
    "fbn_write_csv": [_cstr, _vp, C.c_int, _i64, _vp],
    "fbn_write_libsvm": [_cstr, _vp, _i64, C.c_int, _vp],
    "fbn_dataset_shape": [_vp, _vp, _vp],
    "fbn_dataset_dims": [_vp, _vp],
    "fbn_dataset_columns": [_vp, _vp],
    "fbn_dataset_var_name": [_vp, C.c_int, C.c_char_p, C.c_int],
    "fbn_dataset_destroy": [_vp],
    "fbn_jt_plan_create": [_vp, C.c_int, _pp],
    "fbn_jt_forest_plan_create": [_vp, C.c_int, _pp],
    "fbn_jt_plan_components": [_vp, _vp, _vp],
    "fbn_jt_plan_info_get": [_vp, _vp],
    "fbn_jt_plan_dump": [_vp, _cstr, _cstr],
    "fbn_jt_run": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_jt_run_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_jt_evidence_validate": [_vp, _vp, _i64, _vp],
    "fbn_jt_set_evidence_check": [_vp, C.c_int],
    "fbn_jt_set_kernel_timing": [_vp, C.c_int],
    "fbn_jt_score": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_jt_set_output_layout": [_vp, C.c_int],
    "fbn_jt_score_terms_device": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_jt_last_kernel_ms": [_vp, _vp],
    "fbn_jt_stream_schedule": [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp],
    "fbn_jt_set_waves_per_cu": [_vp, C.c_int],
    "fbn_jt_set_variant": [_vp, C.c_int],
    "fbn_jt_debug_op_cycles": [_vp, C.c_int, _vp],
    "fbn_jt_kernel_source": [_vp, C.c_char_p, C.c_int64, _vp],
    "fbn_jt_kernel_cache_path": [_vp, C.c_char_p, C.c_int64],
    "fbn_jt_kernel_options": [C.c_char_p, C.c_int64],
    "fbn_jt_kernel_build": [_vp],
    "fbn_jt_kernel_placement": [_vp, _vp],
    "fbn_jt_debug_force_fixup": [_vp, C.c_int],
    "fbn_jt_debug_flagged_blocks": [_vp, _vp],
    "fbn_jt_set_exact": [_vp, C.c_int],
    "fbn_jt_plan_destroy": [_vp],
    "fbn_ci_dataset_upload": [_vp, C.c_int, _i64, _vp, C.c_int, _pp],
    "fbn_ci_dataset_from_device": [_vp, C.c_int, _i64, _vp, C.c_int, _pp],
    "fbn_ci_set_kernel_timing": [_vp, C.c_int],
    "fbn_ci_run": [_vp, _vp, _i64, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "fbn_ci_counts": [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _i64, _vp],
    "fbn_ci_last_kernel_ms": [_vp, _vp],
    "fbn_ci_decision_margin": [_vp, _vp, _vp, C.c_int],
    "fbn_ci_debug_counts": [_vp, _vp, _i64, C.c_int, _vp, _i64],
    "fbn_ci_level0_info": [_vp, _vp],
    "fbn_ci_debug_level0_range": [_vp, _i64, _i64, _vp],
    "fbn_pc_decision_margin": [_vp, _vp, _vp],
    "fbn_ci_ctx_destroy": [_vp],
    "fbn_pc_stable": [_vp, _dbl, C.c_int, C.c_int, _pp],
    "fbn_pc_num_levels": [_vp, _vp],
    "fbn_pc_level_tests": [_vp, _vp],
    "fbn_pc_level_launched": [_vp, _vp],
    "fbn_pc_num_edges": [_vp, _vp],
    "fbn_pc_edges": [_vp, _vp],
    "fbn_pc_sepsets": [_vp, _vp, _i64, _vp],
    "fbn_pc_timing": [_vp, _vp, _vp],
    "fbn_pc_path": [_vp, _vp],
    "fbn_jt_tile_program": [_vp, _vp, _vp, _vp, _vp],
    "fbn_pc_result_record": [_vp, _vp, C.c_int64, _vp],
    "fbn_pc_small_eligible": [_vp, C.c_int, _vp],
    "fbn_pc_small_eligible_shape": [C.c_int, C.c_int64, _vp, C.c_int, _vp],
    "fbn_pc_device_bytes": [_vp, _vp],
    "fbn_pc_orient_skeleton": [C.c_int, _vp, C.c_int, _vp, C.c_int64, _vp],
    "fbn_pc_level": [_vp, C.c_double, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp],
    "fbn_pc_num_oriented_edges": [_vp, _vp],
    "fbn_pc_oriented_edges": [_vp, _vp],
    "fbn_pc_shd_bif": [_vp, C.c_char_p, _vp],
    "fbn_shd_bif": [C.c_char_p, C.c_int, _vp, C.c_int, _vp],
    "fbn_pc_result_destroy": [_vp],
    "fbn_pc_dist_create": [C.c_int, _dbl, C.c_int, C.c_int, _pp],
    "fbn_pc_dist_level": [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp],
    "fbn_pc_dist_num_edges": [_vp, _vp],
    "fbn_pc_dist_edges": [_vp, _vp, _i64],
    "fbn_pc_dist_run": [_vp, _vp, _vp],
    "fbn_pc_dist_pack": [_vp, _vp, _vp, _i64, _i64, _vp],
    "fbn_pc_dist_pairs_chunk": [_vp, _vp],
    "fbn_pc_dist_pairs_export": [_vp, _vp, C.c_int],
    "fbn_pc_dist_pairs_import": [_vp, _vp, _vp, C.c_int],
    "fbn_pc_dist_apply": [_vp, _vp, _vp],
    "fbn_pc_dist_result": [_vp, _pp],
    "fbn_pc_dist_destroy": [_vp],
    "fbn_param_family_sizes": [C.c_int, _vp, _vp, _vp, _vp, _vp],
    "fbn_param_counts": [_vp, _vp, _vp, _vp, _i64, _vp],
    "fbn_param_learn": [_vp, _vp, _vp, _vp, _pp],
    "fbn_param_set_tuning": [_vp, _i64, _i64],
    "fbn_pdag_to_dag": [C.c_int, _vp, C.c_int, _vp, _vp],
    "fbn_sampler_create": [_vp, C.c_int, _pp],
    "fbn_sampler_destroy": [_vp],
    "fbn_sample_forward": [_vp, _i64, C.c_uint64, _vp],
    "fbn_sample_forward_device": [_vp, _i64, C.c_uint64, _vp, _vp],
    "fbn_lw_run": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_lw_run_device": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp, _vp],
    "fbn_lw_debug_samples": [_vp, C.c_int, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_sampler_last_kernel_ms": [_vp, _vp],
    "fbn_score_marginals": [_vp, _vp, _vp, _i64, _vp, _vp],
    "fbn_lbp_create": [_vp, C.c_int, _pp],
    "fbn_lbp_destroy": [_vp],
    "fbn_lbp_info": [_vp, _vp, _vp, _vp, _vp],
    "fbn_lbp_run": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp, _vp],
    "fbn_lbp_run_device": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_lbp_debug_messages": [_vp, _vp, _i64, C.c_int, _dbl, _vp],
    "fbn_lbp_set_tuning": [_vp, _i64, C.c_int],
    "fbn_lbp_last_kernel_ms": [_vp, _vp],
    "fbn_epis_create": [_vp, C.c_int, _pp],
    "fbn_epis_destroy": [_vp],
    "fbn_epis_run": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp],
    "fbn_epis_run_device": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_epis_debug_samples": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, C.c_int, _dbl, _dbl, _dbl, _vp, _vp, _vp, _vp],
    "fbn_epis_set_tuning": [_vp, _i64],
    "fbn_epis_info": [_vp, _vp, _vp],
    "fbn_epis_last_kernel_ms": [_vp, _vp, _vp],
    "fbn_ais_create": [_vp, C.c_int, _pp],
    "fbn_ais_destroy": [_vp],
    "fbn_ais_run": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp],
    "fbn_ais_run_device": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp, _vp],
    "fbn_ais_debug_samples": [_vp, C.c_int, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _dbl, _vp, _vp, _vp, _vp],
    "fbn_ais_set_tuning": [_vp, _i64, C.c_int],
    "fbn_ais_info": [_vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_ais_last_kernel_ms": [_vp, _vp],
    "fbn_ais_eta": [C.c_int, C.c_int, _vp],
    "fbn_mpe_create": [_vp, C.c_int, _pp],
    "fbn_mpe_destroy": [_vp],
    "fbn_mpe_info": [_vp, _vp, _vp, _vp, _vp],
    "fbn_mpe_run": [_vp, _vp, _i64, _vp, _vp],
    "fbn_mpe_run_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_mpe_debug_messages": [_vp, _vp, _i64, _vp, _vp],
    "fbn_mpe_set_tuning": [_vp, C.c_int, _i64],
    "fbn_mpe_last_kernel_ms": [_vp, _vp],
    "fbn_em_create": [_vp, C.c_int, _pp],
    "fbn_em_destroy": [_vp],
    "fbn_em_info": [_vp, _vp, _vp, _vp, _vp, _vp],
    "fbn_em_estep": [_vp, _vp, _i64, _vp, _vp],
    "fbn_em_estep_device": [_vp, _vp, _i64, _vp, _vp, _vp],
    "fbn_em_run": [_vp, _vp, _i64, C.c_int, _dbl, _dbl, _vp, _vp],
    "fbn_em_set_parameters": [_vp, _vp],
    "fbn_em_network": [_vp, _pp],
    "fbn_em_debug_posteriors": [_vp, _vp, _i64, _vp],
    "fbn_em_set_tuning": [_vp, C.c_int, _i64],
    "fbn_em_last_kernel_ms": [_vp, _vp],
    "fbn_psample_create": [_vp, C.c_int, _pp],
    "fbn_psample_destroy": [_vp],
    "fbn_psample_info": [_vp, _vp, _vp, _vp, _vp],
    "fbn_psample_run": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp],
    "fbn_psample_run_device": [_vp, _vp, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_psample_set_tuning": [_vp, C.c_int, _i64, _i64],
    "fbn_psample_last_kernel_ms": [_vp, _vp],
    "fbn_gibbs_create": [_vp, C.c_int, _pp],
    "fbn_gibbs_destroy": [_vp],
    "fbn_gibbs_run": [_vp, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp],
    "fbn_gibbs_run_device": [_vp, _vp, _i64, _i64, _i64, _i64, C.c_uint64, _i64, _vp, _vp, _vp, _vp],
    "fbn_gibbs_set_tuning": [_vp, _i64, C.c_int, C.c_int],
    "fbn_gibbs_info": [_vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "fbn_gibbs_last_kernel_ms": [_vp, _vp],
    "fbn_gibbs_debug_conditionals": [_vp, _vp, _i64, _vp],
    "fbn_hc_table_bytes": [_i64, _vp],
    "fbn_hc_penalty": [_cstr, _i64, _vp],
    "fbn_score_families": [_vp, _dbl, _i64, _vp, _vp, _vp, _vp],
    "fbn_score_families_host": [C.c_int, _vp, _vp, _i64, _dbl, _i64, _vp, _vp, _vp, _vp],
    "fbn_hc_set_tuning": [_vp, _i64],
    "fbn_hc_run": [_vp, _vp, _pp],
    "fbn_hc_run_host": [C.c_int, _vp, _vp, _i64, _vp, _pp],
    "fbn_hc_result_info": [_vp, _vp],
    "fbn_hc_result_parents": [_vp, _vp, _vp],
    "fbn_hc_result_node_scores": [_vp, _vp, _vp],
    "fbn_hc_result_trace": [_vp, _vp, _vp],
    "fbn_hc_result_destroy": [_vp],
    "fbn_exact_run": [_vp, _vp, _pp],
    "fbn_exact_run_host": [C.c_int, _vp, _vp, _i64, _vp, _pp],
    "fbn_exact_result_info": [_vp, _vp],
    "fbn_exact_set_tuning": [_vp, _i32],
    "fbn_score_families_bd": [_vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_score_families_bd_host": [C.c_int, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_hc_run_bd": [_vp, _vp, _vp, _pp],
    "fbn_hc_run_bd_host": [C.c_int, _vp, _vp, _i64, _vp, _vp, _pp],
    "fbn_exact_run_bd": [_vp, _vp, _vp, _pp],
    "fbn_exact_run_bd_host": [C.c_int, _vp, _vp, _i64, _vp, _vp, _pp],
    "fbn_bd_set_tuning": [_vp, _i32],
    "fbn_bd_lgamma_diff": [_i64, _dbl, _vp, _vp],
    "fbn_bd_score_table_host": [_vp, _i32, _i32, _vp, _vp, _vp],
    "fbn_bma_run": [_vp, _vp, _i32, _pp],
    "fbn_bma_run_host": [C.c_int, _vp, _vp, _i64, _vp, _i32, _pp],
    "fbn_bma_run_bd": [_vp, _vp, _i32, _vp, _pp],
    "fbn_bma_run_bd_host": [C.c_int, _vp, _vp, _i64, _vp, _i32, _vp, _pp],
    "fbn_bma_result_info": [_vp, _vp],
    "fbn_bma_result_arcs": [_vp, _vp, _vp],
    "fbn_bma_result_destroy": [_vp],
    "fbn_bma_set_tuning": [_vp, _i32],
    "fbn_bma_lse_exp": [_dbl, _vp],
    "fbn_bma_lse": [_dbl, _dbl, _vp],
    "fbn_omcmc_run": [_vp, _vp, _i32, _vp, _pp],
    "fbn_omcmc_run_bd": [_vp, _vp, _i32, _vp, _vp, _pp],
    "fbn_omcmc_run_host": [C.c_int, _vp, _vp, _i64, _vp, _i32, _vp, _pp],
    "fbn_omcmc_run_bd_host": [C.c_int, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _pp],
    "fbn_omcmc_result_info": [_vp, _vp],
    "fbn_omcmc_result_arcs": [_vp, _vp, _vp, _vp, _vp, _vp],
    "fbn_omcmc_result_destroy": [_vp],
    "fbn_omcmc_set_tuning": [_vp, _i32, _i64],
    "fbn_omcmc_order_terms": [_vp, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp],
    "fbn_omcmc_order_terms_host": [C.c_int, _vp, _vp, _i64, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp],
    "fbn_cdataset_load_csv": [_cstr, _pp],
    "fbn_cdataset_shape": [_vp, _vp, _vp],
    "fbn_cdataset_columns": [_vp, _vp],
    "fbn_cdataset_var_name": [_vp, C.c_int, C.c_char_p, C.c_int],
    "fbn_cdataset_destroy": [_vp],
    "fbn_gci_upload": [_vp, C.c_int, _i64, C.c_int, _pp],
    "fbn_gci_from_device": [_vp, C.c_int, _i64, C.c_int, _pp],
    "fbn_gci_corr": [_vp, _vp],
    "fbn_gci_run": [_vp, _vp, _i64, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "fbn_gci_pc_stable": [_vp, _dbl, C.c_int, _pp],
    "fbn_pc_degenerate": [_vp, _vp],
    "fbn_gci_set_tuning": [_vp, _i32, _i32],
    "fbn_gci_info": [_vp, _vp],
    "fbn_gci_last_kernel_ms": [_vp, _vp],
    "fbn_gci_corr_kernel_ms": [_vp, _vp],
    "fbn_gci_ctx_destroy": [_vp],
    "fbn_gci_host_run": [_vp, C.c_int, _i64, _vp, _i64, C.c_int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "fbn_gci_host_pc_stable": [_vp, C.c_int, _i64, _dbl, C.c_int, _pp],
    "fbn_gci_tau": [_dbl, _i64, C.c_int, _vp],
    "fbn_gci_moments": [_vp, _vp, _vp, _vp],
    "fbn_gscore_families": [_vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_gscore_families_host": [C.c_int, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "fbn_hc_run_gauss": [_vp, _vp, _vp, _pp],
    "fbn_hc_run_gauss_host": [C.c_int, _i64, _vp, _vp, _vp, _vp, _pp],
    "fbn_gscore_info": [_vp, _vp],
    "fbn_gnet_create": [C.c_int, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_gnet_learn": [_vp, _vp, _vp, _pp],
    "fbn_gnet_learn_host": [C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, _pp],
    "fbn_gnet_params": [_vp, _vp, _vp, _vp],
    "fbn_gnet_joint": [_vp, _vp, _vp],
    "fbn_gnet_destroy": [_vp],
    "fbn_ginf_create": [_vp, C.c_int, _pp],
    "fbn_ginf_run": [_vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_ginf_run_device": [_vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fbn_ginf_set_tuning": [_vp, _i32],
    "fbn_ginf_info": [_vp, _vp],
    "fbn_ginf_last_kernel_ms": [_vp, _vp],
    "fbn_ginf_destroy": [_vp],
}


class FastBNError(RuntimeError):
    pass


class _Lib:
    """Lazily loaded libfastbn.so.  Missing library => every call raises (no CPU fallback)."""

    def __init__(self):
        self._h = None

    def load(self):
        if self._h is None:
            if not os.path.exists(LIB_PATH):
                raise FastBNError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback)")
            try:
                # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's): load it first
                # so that one HIP runtime serves both when they share a process
                import torch  # noqa: F401
            except ImportError:
                pass
            h = C.CDLL(LIB_PATH)
            for name, args in _SIGS.items():
                f = getattr(h, name)
                f.argtypes = args
                f.restype = C.c_int
            h.fbn_last_error.restype = C.c_char_p
            h.fbn_last_error.argtypes = []
            self._h = h
        return self._h

    def __getattr__(self, name):
        h = self.load()
        f = getattr(h, name)
        if name == "fbn_last_error":
            return f

        def call(*args):
            rc = f(*args)
            if rc != 0:
                err = FastBNError(f"{name}: {h.fbn_last_error().decode()} (code {rc})")
                err.code = rc  # the fbn_err_t value (include/fastbn.h)
                raise err
            return rc

        return call


lib = _Lib()

# Every live handle (networks, datasets, plans, CI contexts, results, sessions) is destroyed by an
# atexit hook, before the interpreter's module teardown and before the HIP runtime's own exit
# handlers: no fbn_* destroy ever runs from a finalizer racing those (or after `lib` is gone).
# Destroy order: results and sessions, then plans and contexts (they drain their device work),
# then host-only handles.
_LIVE = weakref.WeakSet()
_CLOSE_ORDER = {"PCResult": 0, "PCDistSession": 1, "JunctionTree": 2, "Sampler": 2, "LikelihoodWeighting": 2,
                "LoopyBeliefPropagation": 2, "EPISBN": 2, "AISBN": 2, "SelfImportanceSampling": 2, "MostProbableExplanation": 2,
                "ExpectationMaximization": 2, "PosteriorSampler": 2, "GibbsSampling": 2, "GaussianInference": 2,
                "IndependenceTest": 3, "GaussianIndependenceTest": 3, "Dataset": 4, "Network": 5, "GaussianNetwork": 5}


def _register(obj):
    _LIVE.add(obj)


def close_all():
    """Destroy every live handle now (also run at interpreter exit)."""
    objs = sorted(list(_LIVE), key=lambda o: _CLOSE_ORDER.get(type(o).__name__, 9))
    for o in objs:
        try:
            o.close()
        except Exception:  # noqa: BLE001 (exit path: keep closing the rest)
            pass


atexit.register(close_all)


class _Handle:
    """A libfastbn handle: `_h`, destroyed once by close() (explicitly, by __del__, or at exit)."""
    _destroy = None

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            getattr(lib, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (finalizer)
            pass


def _p(a):
    return None if a is None else a.ctypes.data


def device_count():
    n = C.c_int(0)
    lib.fbn_device_count(C.byref(n))
    return n.value


class _PlanInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_cliques", C.c_int32), ("num_separators", C.c_int32),
                ("num_levels", C.c_int32), ("root", C.c_int32), ("sum_dom", C.c_int32),
                ("clique_entries", C.c_int64), ("separator_entries", C.c_int64),
                ("algorithmic_bytes_per_case", C.c_int64), ("num_ops", C.c_int32),
                ("max_vars_per_table", C.c_int32), ("specialized_eligible", C.c_int32),
                ("variant", C.c_int32), ("streamed_eligible", C.c_int32), ("streamed_waves", C.c_int32),
                ("streamed_split_efficiency", C.c_double), ("tiled_eligible", C.c_int32),
                ("tiled_passes", C.c_int32), ("tiled_entry_visits", C.c_int64), ("tiled_lds_bytes", C.c_int64),
                ("tiled_table_bytes", C.c_int64)]


class Network(_Handle):
    """Discrete BN loaded from XMLBIF (CustomNetwork::GetNetFromXMLBIFFile)."""

    _destroy = "fbn_network_destroy"

    def __init__(self, path=None, _handle=None):
        h = C.c_void_p() if _handle is None else _handle
        if _handle is None:
            lib.fbn_network_load_xmlbif(os.fsencode(path), C.byref(h))
        self._h = h
        _register(self)
        n = C.c_int()
        lib.fbn_network_num_nodes(h, C.byref(n))
        self.num_nodes = n.value
        self.dims = np.zeros(self.num_nodes, np.int32)
        lib.fbn_network_dims(h, _p(self.dims))

    @classmethod
    def from_counts(cls, dims, parents, counts, names=None):
        """A network built in memory (fbn_network_create; the reference's Network of DiscreteNodes,
        src/DiscreteNode.cpp:114-147): dims[v] states, parents[v] (the node's own order), counts[v]
        = int [dims[v]][parent configs], configurations over the parents in ascending index order,
        last fastest (map_cond_prob_table_statistics)."""
        n = len(dims)
        d = np.ascontiguousarray(dims, np.int32)
        off = np.zeros(n + 1, np.int32)
        for v in range(n):
            off[v + 1] = off[v] + len(parents[v])
        par = np.ascontiguousarray([q for ps in parents for q in ps] or [0], np.int32)
        cnt = np.ascontiguousarray(np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in counts]), np.int64)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_network_create(n, _p(d), _p(off), _p(par), _p(cnt), C.cast(nm, C.c_void_p) if nm is not None else None,
                               C.byref(h))
        return cls(_handle=h)

    @classmethod
    def from_cpts(cls, dims, parents, cpts, names=None):
        """A network that holds probabilities (fbn_network_create_cpt): as from_counts with cpts[v] = fp64
        [dims[v]][parent configs]; every entry finite and > 0, every column summing to 1 within 1e-9."""
        n = len(dims)
        d = np.ascontiguousarray(dims, np.int32)
        off = np.zeros(n + 1, np.int32)
        for v in range(n):
            off[v + 1] = off[v] + len(parents[v])
        par = np.ascontiguousarray([q for ps in parents for q in ps] or [0], np.int32)
        tab = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1) for c in cpts]), np.float64)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_network_create_cpt(n, _p(d), _p(off), _p(par), _p(tab),
                                   C.cast(nm, C.c_void_p) if nm is not None else None, C.byref(h))
        return cls(_handle=h)

    def node_probs(self, v):
        """(parents ascending, probabilities fp64 [dims[v]][parent configs]) of node v: a probability
        network's entries, or a count network's (count + 1) / (total + dims[v])."""
        npar, n = C.c_int(), C.c_int64()
        lib.fbn_network_node_probs(self._h, int(v), None, None, C.byref(npar), C.byref(n))
        par = np.zeros(max(1, npar.value), np.int32)
        pr = np.zeros(max(1, n.value), np.float64)
        lib.fbn_network_node_probs(self._h, int(v), _p(par), _p(pr), C.byref(npar), C.byref(n))
        return par[:npar.value], pr[:n.value].reshape(int(self.dims[v]), -1)

    def node_counts(self, v):
        """(parents ascending, counts [dims[v]][parent configs]) of node v."""
        npar, ncnt = C.c_int(), C.c_int64()
        lib.fbn_network_node_counts(self._h, int(v), None, None, C.byref(npar), C.byref(ncnt))
        par = np.zeros(max(1, npar.value), np.int32)
        cnt = np.zeros(max(1, ncnt.value), np.int64)
        lib.fbn_network_node_counts(self._h, int(v), _p(par), _p(cnt), C.byref(npar), C.byref(ncnt))
        return par[:npar.value], cnt[:ncnt.value].reshape(int(self.dims[v]), -1)

    def name(self, i):
        buf = C.create_string_buffer(256)
        lib.fbn_network_name(self._h, i, buf, 256)
        return buf.value.decode()

    def forward_sample(self, n, seed):
        """n complete cases, uint8 [V][n] (fbn_synth_forward_sample; = synth.forward_sample)."""
        cols = np.empty((self.num_nodes, n), np.uint8)
        lib.fbn_synth_forward_sample(self._h, int(n), int(seed), _p(cols))
        return cols

    def evidence_cases(self, n, k, seed, query=0):
        """n evidence cases observing k variables each, int8 [n][V] (fbn_synth_evidence; =
        synth.evidence_cases)."""
        ev = np.empty((n, self.num_nodes), np.int8)
        lib.fbn_synth_evidence(self._h, int(n), int(k), int(seed), int(query), _p(ev))
        return ev



def write_csv(path, columns, network=None):
    """CSV of a column store (header + "s<code>" values), the reference's LoadCSVData input."""
    cols = np.ascontiguousarray(columns, np.uint8)
    lib.fbn_write_csv(os.fsencode(path), _p(cols), cols.shape[0], cols.shape[1], network._h if network else None)


def write_libsvm(path, evidence, labels=None):
    """LIBSVM test set of evidence rows (label + observed v:x), the reference's
    LoadLIBSVMDataKnownNetwork input."""
    ev = np.ascontiguousarray(evidence, np.int8)
    lab = None if labels is None else np.ascontiguousarray(labels, np.int32)
    lib.fbn_write_libsvm(os.fsencode(path), _p(ev), ev.shape[0], ev.shape[1], None if lab is None else _p(lab))


def kernel_options():
    """Compile options of the plan-specialized JT kernel (list of str)."""
    buf = C.create_string_buffer(1024)
    lib.fbn_jt_kernel_options(buf, 1024)
    return [x for x in buf.value.decode().split("\n") if x]


def load_libsvm(path, num_nodes):
    """Dataset::LoadLIBSVMDataKnownNetwork + Inference evidence extraction -> (evidence, labels)."""
    n = C.c_int64()
    lib.fbn_evidence_load_libsvm(os.fsencode(path), num_nodes, None, None, 0, C.byref(n))
    ev = np.zeros((n.value, num_nodes), np.int8)
    lab = np.zeros(n.value, np.int32)
    lib.fbn_evidence_load_libsvm(os.fsencode(path), num_nodes, _p(ev), _p(lab), n.value, C.byref(n))
    return ev, lab


class Dataset:
    """CSV training set with first-appearance value coding (Dataset::LoadCSVData)."""

    def __init__(self, path=None, columns=None, dims=None):
        if path is not None:
            h = C.c_void_p()
            lib.fbn_dataset_load_csv(os.fsencode(path), C.byref(h))
            nv, ns = C.c_int(), C.c_int64()
            lib.fbn_dataset_shape(h, C.byref(nv), C.byref(ns))
            self.dims = np.zeros(nv.value, np.int32)
            self.columns = np.zeros((nv.value, ns.value), np.uint8)
            lib.fbn_dataset_dims(h, _p(self.dims))
            lib.fbn_dataset_columns(h, _p(self.columns))
            self.names = []
            buf = C.create_string_buffer(256)
            for v in range(nv.value):
                lib.fbn_dataset_var_name(h, v, buf, 256)
                self.names.append(buf.value.decode())
            lib.fbn_dataset_destroy(h)
        else:
            self.columns = np.ascontiguousarray(columns, dtype=np.uint8)
            self.dims = np.ascontiguousarray(dims, dtype=np.int32)
            self.names = [str(i) for i in range(self.columns.shape[0])]

    @property
    def num_vars(self):
        return self.columns.shape[0]

    @property
    def num_instance(self):
        return self.columns.shape[1]


class ContinuousDataset:
    """Real-valued training set: `columns` float64 [nvars][nsamples], from a CSV (a header line of names,
    then rows of numbers: fbn_cdataset_load_csv) or from an array."""

    def __init__(self, path=None, columns=None, names=None):
        if path is not None:
            h = C.c_void_p()
            lib.fbn_cdataset_load_csv(os.fsencode(path), C.byref(h))
            nv, ns = C.c_int(), C.c_int64()
            lib.fbn_cdataset_shape(h, C.byref(nv), C.byref(ns))
            self.columns = np.zeros((nv.value, ns.value), np.float64)
            lib.fbn_cdataset_columns(h, _p(self.columns))
            self.names = []
            buf = C.create_string_buffer(256)
            for v in range(nv.value):
                lib.fbn_cdataset_var_name(h, v, buf, 256)
                self.names.append(buf.value.decode())
            lib.fbn_cdataset_destroy(h)
        else:
            self.columns = np.ascontiguousarray(columns, dtype=np.float64)
            if self.columns.ndim != 2:
                raise ValueError("columns: float64 [nvars][nsamples]")
            self.names = list(names) if names is not None else [str(i) for i in range(self.columns.shape[0])]

    @property
    def num_vars(self):
        return self.columns.shape[0]

    @property
    def num_instance(self):
        return self.columns.shape[1]


class JunctionTree(_Handle):
    """Batched JT inference on one device (JunctionTree ctor + PredictUseJTInfer over all cases)."""

    _destroy = "fbn_jt_plan_destroy"
    _create = "fbn_jt_plan_create"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        getattr(lib, self._create)(network._h, device, C.byref(h))
        self._h = h
        _register(self)
        self.output_layout = 0
        info = _PlanInfo()
        lib.fbn_jt_plan_info_get(h, C.byref(info))
        self.info = {k: getattr(info, k) for k, _ in _PlanInfo._fields_}

    def tile_program(self):
        """The tiled kernel's program (variant 5): (passes [n][32] int32, tab int32, initv fp64,
        geometry dict) -- for host-side checks of its tables (tests/tile_emulator.py)."""
        g = np.zeros(8, np.int64)
        lib.fbn_jt_tile_program(self._h, None, None, None, _p(g))
        passes = np.zeros((int(g[0]), 33), np.int32)
        tab = np.zeros(max(int(g[1]), 1), np.int32)
        iv = np.zeros(max(int(g[2]), 1), np.float64)
        lib.fbn_jt_tile_program(self._h, _p(passes), _p(tab), _p(iv), _p(g))
        keys = ["n_passes", "n_tab", "n_init", "scr_row", "red_row", "store_rows", "cases_per_wave", "slots"]
        return passes, tab, iv, dict(zip(keys, (int(x) for x in g)))

    def dump_plan(self, plan_path, init_path):
        lib.fbn_jt_plan_dump(self._h, os.fsencode(plan_path), os.fsencode(init_path))

    def stream_schedule(self):
        """Streamed-kernel schedule: (order, sched) -- see fbn_jt_stream_schedule."""
        no, ns = C.c_int64(), C.c_int64()
        lib.fbn_jt_stream_schedule(self._h, None, 0, None, 0, C.byref(no), C.byref(ns))
        order = np.zeros(no.value, np.int32)
        sched = np.zeros(ns.value, np.int32)
        lib.fbn_jt_stream_schedule(self._h, _p(order), no.value, _p(sched), ns.value, None, None)
        return order, sched

    def set_waves_per_cu(self, w):
        lib.fbn_jt_set_waves_per_cu(self._h, w)

    def op_cycles(self, enable, read=True):
        """Diagnostic per-op-type cycles of the last run (LDS variant)."""
        buf = np.zeros(10, np.uint64)
        lib.fbn_jt_debug_op_cycles(self._h, int(enable), _p(buf) if read else None)
        names = ["INIT", "MUL", "SEPCOL", "STORE", "LOAD", "DMUL", "SEPDIS", "MARG", "EVZERO", "-"]
        return dict(zip(names, buf.tolist()))

    def kernel_source(self):
        """Source of the plan-specialized kernel (variant 3)."""
        n = C.c_int64()
        lib.fbn_jt_kernel_source(self._h, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value)
        lib.fbn_jt_kernel_source(self._h, buf, n.value, C.byref(n))
        return buf.value.decode()

    def kernel_cache_path(self):
        buf = C.create_string_buffer(4096)
        lib.fbn_jt_kernel_cache_path(self._h, buf, 4096)
        return buf.value.decode()

    def debug_force_fixup(self, enable):
        lib.fbn_jt_debug_force_fixup(self._h, int(enable))

    def debug_flagged_blocks(self):
        """64-case blocks the last run flagged for the exact fixup (variants 3-5)."""
        n = C.c_int64()
        lib.fbn_jt_debug_flagged_blocks(self._h, C.byref(n))
        return n.value

    def set_exact(self, exact):
        """Arithmetic order of the specialized / streamed kernels: True = the reference's
        (bit-identical), False = fast (normalizations that cancel left out; labels equal, marginals
        within 1e-12), None = auto (fast)."""
        lib.fbn_jt_set_exact(self._h, -1 if exact is None else int(bool(exact)))

    def build_kernel(self):
        """Compile the plan-specialized kernel into the on-disk cache (no GPU needed)."""
        lib.fbn_jt_kernel_build(self._h)
        return self.kernel_cache_path()

    def refresh_info(self):
        info = _PlanInfo()
        lib.fbn_jt_plan_info_get(self._h, C.byref(info))
        self.info = {k: getattr(info, k) for k, _ in _PlanInfo._fields_}
        if self.info["specialized_eligible"]:
            # where the specialized kernel of the current order / layout keeps its message rows
            rows = np.zeros(8, np.int64)
            lib.fbn_jt_kernel_placement(self._h, _p(rows))
            names = ("global_collect", "global_distribute", "lds_collect", "lds_distribute", "reg_collect",
                     "reg_distribute", "workspace", "lds_pool")
            self.info.update({"place_rows_" + k: int(v) for k, v in zip(names, rows)})
        return self.info

    def set_variant(self, v):
        """-1 auto, 0 = clique-in-LDS interpreter, 1 = global-workspace interpreter,
        2 = LDS interpreter with IEEE division, 3 = plan-specialized kernel,
        4 = streamed (virtual-table) kernel for large trees, 5 = per-case evidence-reduced
        kernel for large trees (fast arithmetic order)."""
        lib.fbn_jt_set_variant(self._h, v)

    def infer(self, evidence, marginals=True):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None)."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        labels = np.zeros(n, np.int32)
        marg = np.zeros((n, self.info["sum_dom"]), np.float64) if marginals else None
        lib.fbn_jt_run(self._h, _p(ev), n, _p(labels), _p(marg), None)
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, stream_ptr=None):
        """Device-resident run (asynchronous on the stream unless the evidence check is on)."""
        lib.fbn_jt_run_device(self._h, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, stream_ptr)

    def validate_device(self, d_evidence_ptr, ncases, stream_ptr=None):
        """Device-side evidence range check of a device buffer; raises FastBNError if a code is out
        of its node's domain."""
        lib.fbn_jt_evidence_validate(self._h, d_evidence_ptr, ncases, stream_ptr)

    def set_kernel_timing(self, enable):
        """fbn_jt_set_kernel_timing: enable = False records no timing events per run (last_kernel_ms
        then raises); for callers that time with their own events."""
        lib.fbn_jt_set_kernel_timing(self._h, int(bool(enable)))

    def set_evidence_check(self, enable):
        """run_device's per-call evidence check (default on); off = fully asynchronous runs of a
        buffer the caller validated (validate_device)."""
        lib.fbn_jt_set_evidence_check(self._h, int(bool(enable)))

    def set_output_layout(self, layout):
        """fbn_jt_set_output_layout: run_device's marginals 0 = case-major [ncases][sum_dom]
        (default), 1 = variable-major [sum_dom][ncases] (each store writes 64 consecutive cases).
        infer() always returns case-major."""
        lib.fbn_jt_set_output_layout(self._h, int(layout))
        self.output_layout = int(layout)

    def score_terms_device(self, d_marg_ptr, d_golden_ptr, ncases, d_terms_ptr, stream_ptr=None):
        """fbn_jt_score_terms_device: per-case (MSE, HD) terms [ncases][2] fp64 on the device from
        device marginals (the plan's output layout) and a case-major device golden table."""
        lib.fbn_jt_score_terms_device(self._h, d_marg_ptr, d_golden_ptr, ncases, d_terms_ptr, stream_ptr)

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_jt_last_kernel_ms(self._h, C.byref(ms))
        return ms.value

    def score(self, marginals, golden):
        mse, hd = C.c_double(), C.c_double()
        m = np.ascontiguousarray(marginals, np.float64)
        g = np.ascontiguousarray(golden, np.float64)
        lib.fbn_jt_score(self._h, _p(m), _p(g), m.shape[0], C.byref(mse), C.byref(hd))
        return mse.value, hd.value

    def EvaluateAccuracy(self, evidence, ground_truths, golden=None):
        """Accuracy of the query-variable arg-max (+ average MSE/HD vs golden if given)."""
        labels, marg = self.infer(evidence)
        acc = float(np.mean(labels == np.asarray(ground_truths)))
        if golden is None:
            return acc
        mse, hd = self.score(marg, golden)
        return acc, mse / len(labels), hd / len(labels)


class JunctionForest(JunctionTree):
    """JunctionTree for any DAG (fbn_jt_forest_plan_create): where the moral graph is disconnected --
    JunctionTree raises -- one tree per component, none joined to another, so the cost is the sum of
    the trees' and exact inference stays exact.  On a connected network it is JunctionTree's plan.
    components: the moral graph's components as sorted node lists, ordered by their lowest node."""

    _create = "fbn_jt_forest_plan_create"

    def __init__(self, network, device=0):
        super().__init__(network, device)
        comp = np.zeros(self.info["num_nodes"], np.int32)
        n = C.c_int32()
        lib.fbn_jt_plan_components(self._h, _p(comp), C.byref(n))
        self.components = [np.flatnonzero(comp == k).tolist() for k in range(n.value)]


class IndependenceTest(_Handle):
    """G^2 tests on the device (IndependenceTest::IndependenceResult, batched)."""

    _destroy = "fbn_ci_ctx_destroy"

    def __init__(self, dataset, alpha=0.05, device=0):
        self.alpha = alpha
        self.dims = np.ascontiguousarray(dataset.dims, np.int32)
        self.num_samples = int(dataset.num_instance)
        h = C.c_void_p()
        lib.fbn_ci_dataset_upload(_p(dataset.columns), dataset.num_vars, dataset.num_instance,
                                  _p(dataset.dims), device, C.byref(h))
        self._h = h
        _register(self)

    @classmethod
    def from_device(cls, d_cols_ptr, nvars, nsamples, dims, alpha=0.05, device=0):
        """Column store already in `device` memory (uint8 [nvars][nsamples], e.g. a tensor filled by
        an RCCL broadcast): fbn_ci_dataset_from_device."""
        self = cls.__new__(cls)
        self.alpha = alpha
        dims = np.ascontiguousarray(dims, np.int32)
        self.dims = dims
        self.num_samples = int(nsamples)
        h = C.c_void_p()
        lib.fbn_ci_dataset_from_device(C.c_void_p(d_cols_ptr), int(nvars), int(nsamples), _p(dims), device,
                                       C.byref(h))
        self._h = h
        _register(self)
        return self

    def set_kernel_timing(self, enable):
        """HIP-event kernel timing of every CI launch (default on; off saves the events' cost)."""
        lib.fbn_ci_set_kernel_timing(self._h, int(bool(enable)))

    def level(self, d, edges, e_begin, e_end, group_size=1):
        """One skeleton level for edges[e_begin:e_end] of the current skeleton (fbn_pc_level) ->
        (removed[bool], sepsets[list of tuples or None], counted, launched)."""
        ev = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
        n = e_end - e_begin
        rm = np.zeros(max(n, 1), np.uint8)
        sp = np.zeros((max(n, 1), max(d, 1)), np.int32)
        cnt, lau = C.c_int64(), C.c_int64()
        lib.fbn_pc_level(self._h, self.alpha, d, group_size, _p(ev), ev.shape[0], e_begin, e_end, _p(rm), _p(sp),
                         C.byref(cnt), C.byref(lau))
        rm = rm[:n].astype(bool)
        seps = [tuple(int(v) for v in sp[i, :d]) if rm[i] else None for i in range(n)]
        return rm, seps, cnt.value, lau.value

    def run(self, items, d):
        items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 2 + d)
        n = items.shape[0]
        g2 = np.zeros(n)
        df = np.zeros(n, np.int32)
        p = np.zeros(n)
        ind = np.zeros(n, np.uint8)
        lib.fbn_ci_run(self._h, _p(items), n, d, self.alpha, _p(g2), _p(df), _p(p), _p(ind), None)
        return g2, df, p, ind.astype(bool)

    def IndependenceResult(self, x, y, z=()):
        g2, df, p, ind = self.run(np.array([[x, y, *z]], np.int32), len(z))
        return {"g2": g2[0], "df": int(df[0]), "p_value": p[0], "is_independent": bool(ind[0])}

    def production_counts(self, items, d, cap=None):
        """Counts of the tests `items` [n][2+d] through the kernels a PC run uses at level d
        (fbn_ci_debug_counts: level-0 Gram + pair tables, derived level-1 counting, histogram
        kernel) -> int32 [n][cap] (Counts3D order; cells beyond a test's table are 0)."""
        items = np.ascontiguousarray(items, np.int32).reshape(-1, 2 + d)
        if cap is None:
            dims = np.asarray(self.dims)
            cap = int(np.max(np.prod(dims[items], axis=1))) if len(items) else 1
        out = np.zeros((len(items), cap), np.int32)
        lib.fbn_ci_debug_counts(self._h, _p(items), len(items), d, _p(out), cap)
        return out

    def level0_info(self):
        """The last level-0 all-pairs launch of this context (fbn_ci_level0_info): path (1 popcount
        Gram, 2 MFMA Gram, 3 tiled pairs kernel, 0 none yet), R, Rp, KS, nt, S and the shortest /
        longest split-K slice in stages."""
        out = np.zeros(8, np.int64)
        lib.fbn_ci_level0_info(self._h, _p(out))
        keys = ("path", "R", "Rp", "KS", "nt", "S", "shortest", "longest")
        return {k: int(v) for k, v in zip(keys, out)}

    def level0_range_counts(self, pair0, n):
        """The complete-graph pairs [pair0, pair0 + n) as one batch of the PC driver's level-0 chunk
        loop, the level-0 Gram poisoned first (fbn_ci_debug_level0_range) -> int32 [n][16]."""
        out = np.zeros((n, 16), np.int32)
        lib.fbn_ci_debug_level0_range(self._h, int(pair0), int(n), _p(out))
        return out

    def counts(self, x, y, z=()):
        zz = np.array(z, np.int32)
        cells = C.c_int64()
        lib.fbn_ci_counts(self._h, x, y, _p(zz) if len(z) else None, len(z), None, 0, C.byref(cells))
        out = np.zeros(cells.value, np.int32)
        lib.fbn_ci_counts(self._h, x, y, _p(zz) if len(z) else None, len(z), _p(out), cells.value,
                          C.byref(cells))
        return out

    def decision_margin(self, reset=False):
        """(min |p - alpha|, #tests with |p - alpha| < 1e-9) over the tests run since the last reset."""
        m, near = C.c_double(), C.c_int64()
        lib.fbn_ci_decision_margin(self._h, C.byref(m), C.byref(near), int(bool(reset)))
        return m.value, near.value

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_ci_last_kernel_ms(self._h, C.byref(ms))
        return ms.value



def _gci_outputs(n):
    return np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)


class GaussianIndependenceTest(_Handle):
    """Fisher-z tests of the partial correlation on the device (fbn_gci_*): the float64 column store and
    its correlation matrix stay resident."""

    _destroy = "fbn_gci_ctx_destroy"

    def __init__(self, dataset, alpha=0.05, device=0):
        self.alpha = alpha
        self.num_vars, self.num_samples = int(dataset.num_vars), int(dataset.num_instance)
        h = C.c_void_p()
        lib.fbn_gci_upload(_p(dataset.columns), self.num_vars, self.num_samples, device, C.byref(h))
        self._h = h
        _register(self)

    def correlation(self):
        """R float64 [nvars][nvars] as the tests read it: symmetric, unit diagonal."""
        R = np.zeros((self.num_vars, self.num_vars))
        lib.fbn_gci_corr(self._h, _p(R))
        return R

    def run(self, items, d):
        """items [n][2 + d] = (x, y, z...) -> (r, z, p, indep); a degenerate test has r = NaN and is dependent."""
        items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 2 + d)
        n = items.shape[0]
        r, z, p, ind = _gci_outputs(n)
        deg = C.c_int64()
        lib.fbn_gci_run(self._h, _p(items), n, d, self.alpha, _p(r), _p(z), _p(p), _p(ind), C.byref(deg))
        self.degenerate = deg.value
        return r, z, p, ind.astype(bool)

    def IndependenceResult(self, x, y, z=()):
        r, zz, p, ind = self.run(np.array([[x, y, *z]], np.int32), len(z))
        return {"r": r[0], "z": zz[0], "p_value": p[0], "is_independent": bool(ind[0])}

    def set_tuning(self, split_k=0, tile=0):
        """Sample slices and tile edge (32 / 64) of the Gram kernel, 0 = automatic; R is recomputed."""
        lib.fbn_gci_set_tuning(self._h, int(split_k), int(tile))

    def info(self):
        out = np.zeros(4, np.int64)
        lib.fbn_gci_info(self._h, _p(out))
        return {k: int(v) for k, v in zip(("tile", "split_k", "slab_bytes", "degenerate"), out)}

    def moments(self):
        """(mean [n], the centred sums of squares ss [n], R [n][n]) as the context holds them (fbn_gci_moments)."""
        n = self.num_vars
        mean, ss, R = np.zeros(n), np.zeros(n), np.zeros((n, n))
        lib.fbn_gci_moments(self._h, _p(mean), _p(ss), _p(R))
        return mean, ss, R

    def score_info(self):
        """fbn_gscore_info: the last family-score batch."""
        out = np.zeros(3, np.int64)
        lib.fbn_gscore_info(self._h, _p(out))
        return {k: int(v) for k, v in zip(("families", "launches", "degenerate"), out)}

    def corr_kernel_ms(self):
        """(column means, Gram, reduce) of the last computation of R."""
        ms = (C.c_float * 3)()
        lib.fbn_gci_corr_kernel_ms(self._h, ms)
        return tuple(ms)

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_gci_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


def gci_host_run(R, nsamples, items, d, alpha=0.05):
    """The host twin of GaussianIndependenceTest.run on a correlation matrix R (fbn_gci_host_run) ->
    (r, z, p, indep, degenerate count)."""
    R = np.ascontiguousarray(R, np.float64)
    items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 2 + d)
    n = items.shape[0]
    r, z, p, ind = _gci_outputs(n)
    deg = C.c_int64()
    lib.fbn_gci_host_run(_p(R), R.shape[0], int(nsamples), _p(items), n, d, alpha, _p(r), _p(z), _p(p), _p(ind),
                         C.byref(deg))
    return r, z, p, ind.astype(bool), deg.value


def gci_host_pc_stable(R, nsamples, alpha=0.05, depth=1000):
    """The host twin of PC-stable on continuous data over a correlation matrix R -> PCResult."""
    R = np.ascontiguousarray(R, np.float64)
    r = C.c_void_p()
    lib.fbn_gci_host_pc_stable(_p(R), R.shape[0], int(nsamples), alpha, depth, C.byref(r))
    return PCResult(r)


def gci_tau(alpha, nsamples, d):
    """tau_d: a Gaussian test is independent iff |r| <= tau_d."""
    t = C.c_double()
    lib.fbn_gci_tau(alpha, int(nsamples), d, C.byref(t))
    return t.value


class PCResult(_Handle):
    """A PC-stable result handle: skeleton, sepsets, orientation, SHD (fbn_pc_*)."""

    _destroy = "fbn_pc_result_destroy"

    def __init__(self, handle):
        self._h = handle
        _register(self)
        self._edges = self._sepset = self._oriented = None
        m, near = C.c_double(), C.c_int64()
        lib.fbn_pc_decision_margin(handle, C.byref(m), C.byref(near))
        # p-values are parity-unpinned; decisions this close to alpha are flagged
        self.min_margin, self.near_alpha = m.value, near.value
        nl = C.c_int()
        lib.fbn_pc_num_levels(handle, C.byref(nl))
        self.tests_per_level = np.zeros(nl.value, np.int64)
        self.launched_per_level = np.zeros(nl.value, np.int64)
        if nl.value:
            lib.fbn_pc_level_tests(handle, _p(self.tests_per_level))
            lib.fbn_pc_level_launched(handle, _p(self.launched_per_level))
        self.num_ci_test = int(self.tests_per_level.sum())
        tot, ker = C.c_double(), C.c_double()
        lib.fbn_pc_timing(handle, C.byref(tot), C.byref(ker))
        self.total_s, self.kernel_s = tot.value, ker.value
        path = C.c_int()
        lib.fbn_pc_path(handle, C.byref(path))
        # 0 host-driven levels, 1 device-resident search, 2 device-resident search fell back to the host
        self.path = path.value
        nb = C.c_int64()
        lib.fbn_pc_device_bytes(handle, C.byref(nb))
        self.device_bytes = nb.value
        deg = C.c_int64()
        lib.fbn_pc_degenerate(handle, C.byref(deg))
        self.degenerate = deg.value  # Gaussian runs: tests with a singular conditioning block (dependent)

    @classmethod
    def with_levels(cls, handle):
        return cls(handle)

    # skeleton / sepsets / orientation are converted to Python objects on first access (a
    # 1000-variable run has ~500k sepsets: the conversion costs far more than the search)
    @property
    def edges(self):
        if self._edges is None:
            ne = C.c_int()
            lib.fbn_pc_num_edges(self._h, C.byref(ne))
            e = np.zeros((max(ne.value, 1), 2), np.int32)
            if ne.value:
                lib.fbn_pc_edges(self._h, _p(e))
            self._edges = [tuple(map(int, x)) for x in e[:ne.value]]
        return self._edges

    @property
    def sepset(self):
        if self._sepset is None:
            ln = C.c_int64()
            lib.fbn_pc_sepsets(self._h, None, 0, C.byref(ln))
            buf = np.zeros(max(ln.value, 1), np.int32)
            lib.fbn_pc_sepsets(self._h, _p(buf), ln.value, C.byref(ln))
            sep, k, b = {}, 0, buf.tolist()
            while k < ln.value:
                x, y, m = b[k], b[k + 1], b[k + 2]
                sep[(x, y)] = tuple(b[k + 3:k + 3 + m])
                k += 3 + m
            self._sepset = sep
        return self._sepset

    @property
    def oriented(self):
        """(from, to, 1) arcs and (min, max, 0) undirected edges, in vec_edges order."""
        if self._oriented is None:
            no = C.c_int()
            lib.fbn_pc_num_oriented_edges(self._h, C.byref(no))
            t = np.zeros((max(no.value, 1), 3), np.int32)
            if no.value:
                lib.fbn_pc_oriented_edges(self._h, _p(t))
            self._oriented = [tuple(map(int, x)) for x in t[:no.value]]
        return self._oriented

    def GetSHD(self, bif_path):
        """BNSLComparison(ref_net, network).GetSHD() with ref_net loaded from a BIF file."""
        shd = C.c_int()
        lib.fbn_pc_shd_bif(self._h, os.fsencode(bif_path), C.byref(shd))
        return shd.value



def shd_bif(bif_path, nvars, oriented):
    """SHD of a learned graph [(from, to, 1) | (a, b, 0)] vs the CPDAG of a BIF DAG."""
    t = np.ascontiguousarray(np.asarray(oriented if oriented else [(0, 0, 0)], np.int32).reshape(-1, 3))
    shd = C.c_int()
    lib.fbn_shd_bif(os.fsencode(bif_path), int(nvars), _p(t), len(oriented), C.byref(shd))
    return shd.value


def orient_skeleton(nvars, edges, sepset):
    """Host-only orientation of a given skeleton (PCStable steps 2-3) -> PCResult."""
    pairs = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    rec = []
    for (x, y), z in sorted(sepset.items()):
        rec += [x, y, len(z)] + list(z)
    rec = np.ascontiguousarray(np.asarray(rec if rec else [0], np.int32))
    r = C.c_void_p()
    lib.fbn_pc_orient_skeleton(int(nvars), _p(pairs), int(pairs.shape[0]), _p(rec), len(rec) if sepset else 0,
                               C.byref(r))
    return PCResult(r)


class PCStable:
    """PC-stable (PCStable(net, alpha, depth).StructLearnCompData): device skeleton + host orientation."""

    def __init__(self, alpha=0.05, depth=1000, device=0):
        self.alpha, self.depth, self.device = alpha, depth, device
        self.result = None
        self.ci = None

    def StructLearnCompData(self, dataset, group_size=1, num_threads=1, print_struct=False, verbose=False):
        """`dataset`: a Dataset (uploaded for this call) or an IndependenceTest whose column store is
        already resident on the device (reused across calls); or a ContinuousDataset / a
        GaussianIndependenceTest: Fisher-z tests of the partial correlation (group_size must be 1)."""
        if isinstance(dataset, (ContinuousDataset, GaussianIndependenceTest)):
            if group_size != 1:
                raise ValueError("continuous data: group_size must be 1")
            ci = dataset if isinstance(dataset, GaussianIndependenceTest) else GaussianIndependenceTest(dataset, self.alpha, self.device)
            self.ci = ci
            r = C.c_void_p()
            lib.fbn_gci_pc_stable(ci._h, self.alpha, self.depth, C.byref(r))
            return self._take(PCResult(r))
        ci = dataset if isinstance(dataset, IndependenceTest) else IndependenceTest(dataset, self.alpha, self.device)
        self.ci = ci  # the context of the run: ParameterLearning(pc.ci) learns from the same upload
        r = C.c_void_p()
        lib.fbn_pc_stable(ci._h, self.alpha, self.depth, group_size, C.byref(r))
        return self._take(PCResult(r))

    def _take(self, res):
        self.result = res
        self.tests_per_level, self.launched_per_level = res.tests_per_level, res.launched_per_level
        self.total_s, self.kernel_s, self.device_bytes = res.total_s, res.kernel_s, res.device_bytes
        self.num_ci_test = res.num_ci_test
        self.min_margin, self.near_alpha = self.result.min_margin, self.result.near_alpha
        return self

    edges = property(lambda self: self.result.edges)
    sepset = property(lambda self: self.result.sepset)
    oriented = property(lambda self: self.result.oriented)
    path = property(lambda self: self.result.path)  # 0 host levels, 1 device-resident, 2 fell back, 3 host levels after the device level 0 -> 1 hand-off

    def GetSHD(self, bif_path):
        return self.result.GetSHD(bif_path)


def _csr_parents(parents, nvars):
    """List of parent lists -> (parent_off int32 [nvars+1], parents int32) for the C-ABI."""
    if len(parents) != nvars:
        raise FastBNError(f"{len(parents)} parent lists for {nvars} variables")
    off = np.zeros(nvars + 1, np.int32)
    for v in range(nvars):
        off[v + 1] = off[v] + len(parents[v])
    par = np.ascontiguousarray([int(q) for ps in parents for q in ps] or [0], np.int32)
    return off, par


def family_sizes(dims, parents):
    """fbn_param_family_sizes: (family_off int64 [n+1], total cells) of the tables counts[v] =
    [dims[v]][parent configurations]; raises FastBNError for a bad parent list (code -1) or a graph
    past the cell cap (code -6).  Host only."""
    d = np.ascontiguousarray(dims, np.int32)
    off, par = _csr_parents(parents, len(d))
    foff = np.zeros(len(d) + 1, np.int64)
    total = C.c_int64()
    lib.fbn_param_family_sizes(len(d), _p(d), _p(off), _p(par), _p(foff), C.byref(total))
    return foff, total.value


def pdag_to_dag(nvars, oriented):
    """fbn_pdag_to_dag: a consistent DAG extension (Dor & Tarsi) of a PDAG given as PCResult.oriented
    gives it -- (from, to, 1) arcs and (a, b, 0) undirected edges -- as a list of ascending parent
    lists.  Deterministic; raises FastBNError if no extension exists.  Host only."""
    n = len(oriented)
    t = np.ascontiguousarray(np.asarray(oriented if n else [(0, 0, 0)], np.int32).reshape(-1, 3))
    off = np.zeros(int(nvars) + 1, np.int32)
    par = np.zeros(max(n, 1), np.int32)
    lib.fbn_pdag_to_dag(int(nvars), _p(t), n, _p(off), _p(par))
    return [[int(q) for q in par[off[v]:off[v + 1]]] for v in range(int(nvars))]


class ParameterLearning:
    """Maximum-likelihood counts of a known structure from complete data on the device
    (ParameterLearning::LearnParamsKnowStructCompData).  `source`: a Dataset (uploaded here) or an
    IndependenceTest, whose context -- and column store -- is shared, so PC-stable and learning use
    one upload (PCStable.ci after a run)."""

    def __init__(self, source, device=0):
        self.ci = source if isinstance(source, IndependenceTest) else IndependenceTest(source, device=device)
        self.dims = np.ascontiguousarray(self.ci.dims, np.int32)

    def counts(self, parents):
        """Family counts of every node: a list of int64 [dims[v]][parent configurations] arrays
        (configurations over the parents in ascending index order, last fastest), the shape
        Network.node_counts returns."""
        n = len(self.dims)
        off, par = _csr_parents(parents, n)
        total = C.c_int64()
        lib.fbn_param_counts(self.ci._h, _p(off), _p(par), None, 0, C.byref(total))
        buf = np.zeros(max(total.value, 1), np.int64)
        lib.fbn_param_counts(self.ci._h, _p(off), _p(par), _p(buf), total.value, C.byref(total))
        out, o = [], 0
        for v in range(n):
            cells = int(self.dims[v]) * int(np.prod(self.dims[list(parents[v])], dtype=np.int64))
            out.append(buf[o:o + cells].reshape(int(self.dims[v]), -1))
            o += cells
        return out

    def LearnParamsKnowStructCompData(self, parents, names=None):
        """The learned Network (fbn_param_learn): parents[v] in the node's own order."""
        n = len(self.dims)
        off, par = _csr_parents(parents, n)
        nm = None
        if names is not None:
            enc = [os.fsencode(x) for x in names]
            nm = (C.c_char_p * n)(*enc)
        h = C.c_void_p()
        lib.fbn_param_learn(self.ci._h, _p(off), _p(par), C.cast(nm, C.c_void_p) if nm is not None else None,
                            C.byref(h))
        return Network(_handle=h)

    def set_tuning(self, samples_per_slice=0, lds_cells_max=0):
        """fbn_param_set_tuning: samples per (family, slice) work item and the largest table counted
        in LDS; 0 = default."""
        lib.fbn_param_set_tuning(self.ci._h, int(samples_per_slice), int(lds_cells_max))

    def last_kernel_ms(self):
        return self.ci.last_kernel_ms()


class GaussianNetwork(_Handle):
    """A linear-Gaussian network (fbn_gnet): X_v = intercept[v] + sum_k coef[v][k] X_parents[v][k] + N(0,
    variance[v]).  `coef` is a list of lists aligned with `parents`, or flat in the same order."""

    _destroy = "fbn_gnet_destroy"

    def __init__(self, parents=None, intercept=None, coef=None, variance=None, names=None, _handle=None):
        self.parents = [[int(q) for q in ps] for ps in parents]
        self.num_nodes = len(self.parents)
        self.names = list(names) if names is not None else [str(i) for i in range(self.num_nodes)]
        self._off, self._par = _csr_parents(self.parents, self.num_nodes)
        if _handle is None:
            flat = [float(w) for ws in coef for w in (ws if np.ndim(ws) else [ws])]
            if len(flat) != int(self._off[-1]):
                raise FastBNError(f"{len(flat)} coefficients for {int(self._off[-1])} parents")
            b = np.ascontiguousarray(intercept, np.float64)
            s = np.ascontiguousarray(variance, np.float64)
            if len(b) != self.num_nodes or len(s) != self.num_nodes:
                raise FastBNError(f"intercept and variance: one value for each of the {self.num_nodes} nodes")
            _handle = C.c_void_p()
            lib.fbn_gnet_create(self.num_nodes, _p(self._off), _p(self._par), _p(b), _p(np.array(flat or [0.0])), _p(s),
                                C.byref(_handle))
        self._h = _handle
        _register(self)

    def params(self):
        """(intercept [n], coef as a list of arrays aligned with parents, variance [n])."""
        b, s = np.zeros(self.num_nodes), np.zeros(self.num_nodes)
        w = np.zeros(max(int(self._off[-1]), 1))
        lib.fbn_gnet_params(self._h, _p(b), _p(w), _p(s))
        return b, [w[self._off[v]:self._off[v + 1]].copy() for v in range(self.num_nodes)], s

    def joint(self):
        """(mu [n], Sigma [n][n]) of the joint normal distribution."""
        mu, cov = np.zeros(self.num_nodes), np.zeros((self.num_nodes, self.num_nodes))
        lib.fbn_gnet_joint(self._h, _p(mu), _p(cov))
        return mu, cov


def gnet_learn_host(mean, ss, R, nsamples, parents, names=None):
    """The host solve of GaussianParameterLearning from moments handed in (fbn_gnet_learn_host): mean [n], the
    centred sums of squares ss [n] and the correlation matrix R [n][n] of nsamples samples -> GaussianNetwork."""
    mean, ss, R = (np.ascontiguousarray(a, np.float64) for a in (mean, ss, R))
    off, par = _csr_parents(parents, len(mean))
    h = C.c_void_p()
    lib.fbn_gnet_learn_host(len(mean), int(nsamples), _p(mean), _p(ss), _p(R), _p(off), _p(par), C.byref(h))
    return GaussianNetwork(parents, names=names, _handle=h)


class GaussianParameterLearning:
    """Maximum-likelihood parameters of a known structure from complete real-valued data.  `source`: a
    ContinuousDataset (uploaded here) or a GaussianIndependenceTest, whose context -- the column store and its
    moments -- is shared, so PC-stable and learning use one upload (PCStable.ci after a run)."""

    def __init__(self, source, device=0):
        self.ci = source if isinstance(source, GaussianIndependenceTest) else GaussianIndependenceTest(source, device=device)

    def LearnParamsKnowStructCompData(self, parents, names=None):
        """The learned GaussianNetwork (fbn_gnet_learn): parents[v] in the node's own order."""
        off, par = _csr_parents(parents, self.ci.num_vars)
        h = C.c_void_p()
        lib.fbn_gnet_learn(self.ci._h, _p(off), _p(par), C.byref(h))
        return GaussianNetwork(parents, names=names, _handle=h)


class GaussianInference(_Handle):
    """Exact inference in a GaussianNetwork (fbn_ginf): batches of evidence cases conditioned on the resident
    joint, one workgroup per case.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_ginf_destroy"

    def __init__(self, network, device=0):
        self.network = network
        self.degenerate = 0
        h = C.c_void_p()
        lib.fbn_ginf_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def infer(self, evidence, mean=True, var=True):
        """evidence float64 [ncases][num_nodes], NaN = unobserved -> (mean, var, logp); a degenerate case is NaN
        throughout and counted in self.degenerate."""
        ev = np.ascontiguousarray(evidence, np.float64).reshape(-1, self.network.num_nodes)
        n = ev.shape[0]
        m = np.zeros(ev.shape) if mean else None
        v = np.zeros(ev.shape) if var else None
        lp = np.zeros(n)
        deg = C.c_int64()
        lib.fbn_ginf_run(self._h, _p(ev), n, _p(m), _p(v), _p(lp), C.byref(deg))
        self.degenerate = deg.value
        return m, v, lp

    def run_device(self, d_evidence_ptr, ncases, d_mean_ptr=None, d_var_ptr=None, d_logp_ptr=None, stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        opt = lambda q: C.c_void_p(q) if q else None
        lib.fbn_ginf_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), opt(d_mean_ptr), opt(d_var_ptr),
                                opt(d_logp_ptr), stream_ptr)

    def set_tuning(self, max_workgroups=0):
        """fbn_ginf_set_tuning: a cap on the persistent grid, 0 = automatic.  Results do not change."""
        lib.fbn_ginf_set_tuning(self._h, int(max_workgroups))

    def info(self):
        out = np.zeros(6, np.int64)
        lib.fbn_ginf_info(self._h, _p(out))
        return {k: int(v) for k, v in zip(("nvars", "m_max", "lds_bytes", "workgroups", "tile", "degenerate"), out)}

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_ginf_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class _BdScore(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("iss", C.c_double)]


def _bd_score(score):
    """The fbn_bd_score record of "bde" (iss = 1), "k2" or ("bde", iss); None for every other score."""
    name, iss = score if isinstance(score, tuple) and len(score) == 2 else (score, 1.0)
    if name not in ("bde", "k2"):
        return None
    if name == "k2" and isinstance(score, tuple):
        raise FastBNError("k2 takes no equivalent sample size: score=\"k2\"")
    return _BdScore(0 if name == "bde" else 1, 0, float(iss))


def _bd_lgamma_diff(n, a):
    """fbn_bd_lgamma_diff, a testing entry: (D(n, a) = lnGamma(a + n) - lnGamma(a) as the BD scores evaluate
    it, the count from which it takes the Stirling form).  Host only."""
    d, t = C.c_double(), C.c_int32()
    lib.fbn_bd_lgamma_diff(int(n), float(a), C.byref(d), C.byref(t))
    return d.value, t.value


def _bd_score_table(table, score):
    """fbn_bd_score_table_host, a testing entry: the twin's (loglik, score) of one r x q table of counts,
    which unlike a dataset's may be all zeros.  Host only."""
    tab = np.ascontiguousarray(table, np.uint32)
    ll, sc = C.c_double(), C.c_double()
    lib.fbn_bd_score_table_host(_p(tab), tab.shape[0], tab.shape[1], C.byref(_bd_score(score)), C.byref(ll), C.byref(sc))
    return ll.value, sc.value


class _GaussScore(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("alpha_mu", C.c_double), ("alpha_w", C.c_double),
                ("penalty", C.c_double)]


def _is_gauss(source):
    return isinstance(source, (ContinuousDataset, GaussianIndependenceTest))


def _gauss_score(score, nsamples):
    """The fbn_gauss_score record of a score on continuous data: "bic" | "aic" | "loglik" | a number (the
    Gaussian log-likelihood score with that penalty per parameter), "bge" | ("bge", alpha_mu) |
    ("bge", alpha_mu, alpha_w)."""
    name, par = (score[0], tuple(score[1:])) if isinstance(score, tuple) else (score, ())
    if name == "bge":
        if len(par) > 2:
            raise FastBNError("bge takes at most (alpha_mu, alpha_w)")
        return _GaussScore(1, 0, float(par[0]) if par else 1.0, float(par[1]) if len(par) == 2 else 0.0, 0.0)
    if name in ("bde", "k2"):
        raise FastBNError(f"score {score!r} is for discrete data; continuous data takes bic, aic, loglik, a number or bge")
    return _GaussScore(0, 0, 1.0, 0.0, hc_penalty(score, nsamples))


def _host_moments(dataset):
    """(mean, ss, R) that host=True hands the twins: of a ContinuousDataset by numpy; of a GaussianIndependenceTest
    the context's own, downloaded, so the twin repeats the device's bits."""
    if isinstance(dataset, GaussianIndependenceTest):
        return dataset.moments()
    x = dataset.columns
    mean = x.mean(axis=1)
    xc = x - mean[:, None]
    S = xc @ xc.T
    ss = np.ascontiguousarray(np.diag(S))
    R = S / np.sqrt(np.outer(ss, ss))
    R = np.triu(R, 1) + np.triu(R, 1).T + np.eye(len(ss))
    return mean, ss, np.ascontiguousarray(R)


def hc_penalty(score, nsamples):
    """fbn_hc_penalty: the penalty of a named score ("bic", "aic", "loglik"), or a number as it is; 0 under
    a Bayesian Dirichlet score ("bde", "k2", ("bde", iss)), which has no penalty term."""
    if _bd_score(score) is not None:
        return 0.0
    if isinstance(score, str):
        p = C.c_double()
        lib.fbn_hc_penalty(score.encode(), int(nsamples), C.byref(p))
        return p.value
    return float(score)


def hc_table_bytes(nsamples):
    """fbn_hc_table_bytes: bytes of the n ln n table of `nsamples` samples (code -6 past 2^24).  Host only."""
    b = C.c_int64()
    lib.fbn_hc_table_bytes(int(nsamples), C.byref(b))
    return b.value


def _csr_families(families):
    """[(child, parents...)] -> (fam_off int64 [n+1], fam_cols int32) for the C-ABI."""
    off = np.zeros(len(families) + 1, np.int64)
    for f, fam in enumerate(families):
        off[f + 1] = off[f] + len(fam)
    cols = np.ascontiguousarray([int(v) for fam in families for v in fam] or [0], np.int32)
    return off, cols


def family_scores(source, families, penalty=0.0, score=None, host=False):
    """fbn_score_families: (loglik, score) float64 arrays of the families [(child, parent, ...), ...] from
    the column store resident in `source` (an IndependenceTest: on the device), or, for a Dataset,
    fbn_score_families_host: the host twin, bit-identical, no device.  score = "bde" | "k2" | ("bde", iss):
    the Bayesian Dirichlet score instead of loglik - penalty (fbn_score_families_bd and its twin).
    On continuous data (a GaussianIndependenceTest, or a ContinuousDataset, uploaded here; host=True: the twin
    fbn_gscore_families_host over numpy's moments, no device) the Gaussian scores (fbn_gscore_families): score =
    "bic" | "aic" | "loglik" | a number, or `penalty` when score is None, or "bge" | ("bge", alpha_mu[, alpha_w]).
    A degenerate family is -inf twice; their count is left in source.degenerate."""
    off, cols = _csr_families(families)
    n = len(families)
    ll, sc = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    if _is_gauss(source):
        ns = source.num_samples if isinstance(source, GaussianIndependenceTest) else source.num_instance
        g = _gauss_score(float(penalty) if score is None else score, ns)
        if host:
            _, ss, R = _host_moments(source)
            deg = C.c_int64()
            lib.fbn_gscore_families_host(source.num_vars, ns, _p(ss), _p(R), C.byref(g), n, _p(off),
                                         _p(cols), _p(ll), _p(sc), C.byref(deg))
            source.degenerate = deg.value
        else:
            ci = source if isinstance(source, GaussianIndependenceTest) else GaussianIndependenceTest(source)
            lib.fbn_gscore_families(ci._h, C.byref(g), n, _p(off), _p(cols), _p(ll), _p(sc))
            source.degenerate = ci.score_info()["degenerate"]
        return ll[:n], sc[:n]
    bd = None
    if score is not None:
        bd = _bd_score(score)
        if bd is None:
            raise FastBNError(f"unknown Bayesian Dirichlet score {score!r} (bde, k2, (bde, iss))")
    if bd is not None and isinstance(source, IndependenceTest):
        lib.fbn_score_families_bd(source._h, C.byref(bd), n, _p(off), _p(cols), _p(ll), _p(sc))
    elif bd is not None:
        lib.fbn_score_families_bd_host(source.num_vars, _p(source.dims), _p(source.columns), source.num_instance,
                                       C.byref(bd), n, _p(off), _p(cols), _p(ll), _p(sc))
    elif isinstance(source, IndependenceTest):
        lib.fbn_score_families(source._h, float(penalty), n, _p(off), _p(cols), _p(ll), _p(sc))
    else:
        lib.fbn_score_families_host(source.num_vars, _p(source.dims), _p(source.columns), source.num_instance,
                                    float(penalty), n, _p(off), _p(cols), _p(ll), _p(sc))
    return ll[:n], sc[:n]


class _HcOptions(C.Structure):
    _fields_ = [("penalty", C.c_double), ("max_parents", C.c_int32), ("max_iter", C.c_int32),
                ("max_family_cells", C.c_int64), ("allowed", C.c_void_p), ("allowed_len", C.c_int64),
                ("start_off", C.c_void_p), ("start_parents", C.c_void_p)]


class _HcInfo(C.Structure):
    _fields_ = [("nvars", C.c_int32), ("narcs", C.c_int32), ("iterations", C.c_int32), ("pad", C.c_int32),
                ("families_scored", C.c_int64), ("batches", C.c_int64), ("score", C.c_double), ("loglik", C.c_double),
                ("kernel_ms", C.c_double), ("first_sweep_kernel_ms", C.c_double), ("first_sweep_wall_ms", C.c_double),
                ("score_wall_ms", C.c_double), ("wall_ms", C.c_double)]


def _take_hc_result(self, r):
    """The fields of an fbn_hc_result onto `self` (HillClimbing, ExactSearch); destroys r."""
    try:
        info = _HcInfo()
        lib.fbn_hc_result_info(r, C.byref(info))
        n, it = info.nvars, info.iterations
        off, par = np.zeros(n + 1, np.int32), np.zeros(max(info.narcs, 1), np.int32)
        lib.fbn_hc_result_parents(r, _p(off), _p(par))
        ns_, nl = np.zeros(n), np.zeros(n)
        lib.fbn_hc_result_node_scores(r, _p(ns_), _p(nl))
        ops, delta = np.zeros((max(it, 1), 3), np.int32), np.zeros(max(it, 1))
        lib.fbn_hc_result_trace(r, _p(ops), _p(delta))
        if isinstance(self, ExactSearch):
            ex = _ExactInfo()
            lib.fbn_exact_result_info(r, C.byref(ex))
            self.exact_info = {k: getattr(ex, k) for k, _ in _ExactInfo._fields_}
    finally:
        lib.fbn_hc_result_destroy(r)
    self.parents = [[int(q) for q in par[off[v]:off[v + 1]]] for v in range(n)]
    self.score, self.loglik = info.score, info.loglik
    self.node_scores, self.node_logliks = ns_, nl
    self.trace = [(int(ops[k, 0]), int(ops[k, 1]), int(ops[k, 2]), float(delta[k])) for k in range(it)]
    self.iterations, self.families_scored, self.kernel_ms = it, info.families_scored, info.kernel_ms
    self.info = {k: getattr(info, k) for k, _ in _HcInfo._fields_ if k != "pad"}
    return self


class _ExactOptions(C.Structure):
    _fields_ = [("penalty", C.c_double), ("max_parents", C.c_int32), ("pad", C.c_int32), ("max_family_cells", C.c_int64),
                ("allowed", C.c_void_p), ("allowed_len", C.c_int64)]


class _ScoredLearner:
    """What HillClimbing, ExactSearch, ArcPosterior and OrderMCMC share: the candidate options, the data source of a
    run (a Dataset's arrays for the host twin, else a shared IndependenceTest, `.ci`) and the call of the entry
    fbn_<stem>_run[_bd][_host] that the score and `host` select."""

    _Options = _ExactOptions  # the entry's options record
    _BD = object()   # in _call's middle arguments: where the entry takes its fbn_bd_score, if the score is one

    def __init__(self, score, max_parents, max_family_cells, allowed, device):
        self.score_name, self.device = score, device
        self.max_parents, self.max_family_cells, self.allowed = max_parents, max_family_cells, allowed
        self.ci = None

    def _source(self, source, host):
        """(leading arguments of the entry, variables, samples): a Dataset's arrays for the twin, else the context"""
        if host:
            return ((source.num_vars, _p(source.dims), _p(source.columns), source.num_instance), source.num_vars,
                    source.num_instance)
        source = self.ci if source is None else source
        self.ci = source if isinstance(source, IndependenceTest) else IndependenceTest(source, device=self.device)
        return (self.ci._h,), len(self.ci.dims), self.ci.num_samples

    def _options(self, nvars, nsamples, penalty=None):
        """(the options record, the arrays it points into); penalty: None = the score's"""
        o = self._Options()
        o.penalty = hc_penalty(self.score_name, nsamples) if penalty is None else penalty
        o.max_parents = -1 if self.max_parents is None else int(self.max_parents)
        o.max_family_cells = int(self.max_family_cells)
        keep = []
        if self.allowed is not None:
            a = np.ascontiguousarray(np.asarray(self.allowed) != 0, np.uint8)
            keep.append(a)
            o.allowed, o.allowed_len = a.ctypes.data, a.size
        return o, keep

    def _call(self, stem, source, host, *middle):
        """fbn_<stem>_run[_bd][_host](source, options, *middle, result): the result handle"""
        r = C.c_void_p()
        bd = _bd_score(self.score_name)
        lead, nvars, nsamples = self._source(source, host)
        o, keep = self._options(nvars, nsamples)
        name = f"fbn_{stem}_run" + ("_bd" if bd is not None else "") + ("_host" if host else "")
        middle = tuple(C.byref(bd) if a is self._BD else a for a in middle if a is not self._BD or bd is not None)
        getattr(lib, name)(*lead, C.byref(o), *middle, C.byref(r))
        del keep
        return r


class HillClimbing(_ScoredLearner):
    """Score-based structure learning: greedy hill climbing over arc additions, deletions and reversals
    (fbn_hc_run; no reference counterpart).  score: "bic" | "aic" | "loglik" or an explicit non-negative
    penalty per free parameter, or a Bayesian Dirichlet score "bde" (BDeu, iss = 1) | ("bde", iss) | "k2"
    (fbn_hc_run_bd).  allowed: [n][n] mask, allowed[x][y] lets the search add x -> y; start: a DAG
    as parent lists.  learn(source): a Dataset (uploaded here), or an IndependenceTest, whose context is
    shared (`.ci`, as PCStable.ci: ParameterLearning(hc.ci) learns from the same upload); host=True runs
    the host twin (fbn_hc_run_host) on a Dataset, without a device.  On continuous data -- a ContinuousDataset
    or a GaussianIndependenceTest, shared as .ci so GaussianParameterLearning(hc.ci) learns from the same upload --
    "bic" | "aic" | "loglik" | a number mean the Gaussian log-likelihood score and "bge" | ("bge", alpha_mu[,
    alpha_w]) the BGe score (fbn_hc_run_gauss; at most 8 parents); "bde" / "k2" there, and "bge" on discrete
    data, raise FastBNError.  Results: .parents (ascending parent
    lists), .score, .loglik, .node_scores, .trace [(type, from, to, delta)] (type 0 add, 1 delete,
    2 reverse), .iterations, .families_scored, .kernel_ms, .info."""

    OPS = ("add", "delete", "reverse")

    def __init__(self, score="bic", max_parents=None, max_family_cells=0, max_iter=None, allowed=None, start=None,
                 device=0):
        super().__init__(score, max_parents, max_family_cells, allowed, device)
        self.max_iter, self.start = max_iter, start

    _Options = _HcOptions

    def _options(self, nvars, nsamples, penalty=None):
        o, keep = super()._options(nvars, nsamples, penalty)
        o.max_iter = -1 if self.max_iter is None else int(self.max_iter)
        if self.start is not None:
            off, par = _csr_parents(self.start, nvars)
            keep += [off, par]
            o.start_off, o.start_parents = off.ctypes.data, par.ctypes.data
        return o, keep

    def learn(self, source, host=False):
        if _is_gauss(source):
            return self._learn_gauss(source, host)
        if self.score_name == "bge" or (isinstance(self.score_name, tuple) and self.score_name[0] == "bge"):
            raise FastBNError("score bge is for continuous data (a ContinuousDataset or GaussianIndependenceTest)")
        return _take_hc_result(self, self._call("hc", source, host, self._BD))

    def _learn_gauss(self, source, host):
        """learn() on continuous data: fbn_hc_run_gauss on a GaussianIndependenceTest (a ContinuousDataset is
        uploaded into one; either way shared as .ci), or with host=True fbn_hc_run_gauss_host over numpy's moments (of a
        GaussianIndependenceTest: over the context's own, downloaded)."""
        r = C.c_void_p()
        if host:
            ns = source.num_samples if isinstance(source, GaussianIndependenceTest) else source.num_instance
            g = _gauss_score(self.score_name, ns)
            o, keep = self._options(source.num_vars, ns, penalty=0.0)
            _, ss, R = _host_moments(source)
            lib.fbn_hc_run_gauss_host(source.num_vars, ns, _p(ss), _p(R), C.byref(o), C.byref(g), C.byref(r))
        else:
            ci = source if isinstance(source, GaussianIndependenceTest) else GaussianIndependenceTest(source, device=self.device)
            self.ci = ci
            g = _gauss_score(self.score_name, ci.num_samples)
            o, keep = self._options(ci.num_vars, ci.num_samples, penalty=0.0)
            lib.fbn_hc_run_gauss(ci._h, C.byref(o), C.byref(g), C.byref(r))
        del keep
        return _take_hc_result(self, r)

    @property
    def oriented(self):
        """The learned arcs as (from, to, 1) triples, the form shd_bif and pdag_to_dag take."""
        return [(q, v, 1) for v, ps in enumerate(self.parents) for q in ps]

    @staticmethod
    def set_tuning(ci, chunk_cells_max=0):
        """fbn_hc_set_tuning on a context: the most table cells per chunk of a batch; 0 = default."""
        lib.fbn_hc_set_tuning(ci._h, int(chunk_cells_max))

    @staticmethod
    def set_bd_tuning(ci, pack=1):
        """fbn_bd_set_tuning on a context: 1 = the BD reduction packs narrow families into one wave, 0 = one
        wave per family; the same bits either way."""
        lib.fbn_bd_set_tuning(ci._h, int(pack))


class _ExactInfo(C.Structure):
    _fields_ = [("nvars", C.c_int32), ("tile_bits", C.c_int32), ("passes", C.c_int32), ("levels", C.c_int32),
                ("families_scored", C.c_int64), ("batches", C.c_int64), ("lattice_bytes", C.c_int64),
                ("score_kernel_ms", C.c_double), ("transform_kernel_ms", C.c_double), ("sink_kernel_ms", C.c_double),
                ("score_wall_ms", C.c_double), ("upload_wall_ms", C.c_double), ("transform_wall_ms", C.c_double),
                ("sink_wall_ms", C.c_double), ("trace_wall_ms", C.c_double), ("wall_ms", C.c_double)]


class ExactSearch(_ScoredLearner):
    """Exact score-optimal structure learning for up to 26 variables: the globally best DAG under a
    decomposable score by dynamic programming over variable subsets (fbn_exact_run; no reference counterpart).
    score, max_parents, max_family_cells, allowed and learn(source, host) are HillClimbing's, and so are the
    result fields (.parents, .score = the optimum R[V], .loglik, .node_scores, .node_logliks, .oriented;
    .iterations is 0 and .trace empty); .exact_info holds the phase record (families scored, lattice bytes,
    transform passes, kernel and wall ms per phase).  host=True runs the host twin (fbn_exact_run_host) on a
    Dataset, bit-identical, without a device.  `.ci` is shared as HillClimbing.ci is."""

    def __init__(self, score="bic", max_parents=None, max_family_cells=0, allowed=None, device=0):
        super().__init__(score, max_parents, max_family_cells, allowed, device)

    def learn(self, source, host=False):
        return _take_hc_result(self, self._call("exact", source, host, self._BD))

    oriented = HillClimbing.oriented

    @staticmethod
    def set_tuning(ci, tile_bits=0):
        """fbn_exact_set_tuning on a context: bits per pass of the subset-max transform; 0 = default."""
        lib.fbn_exact_set_tuning(ci._h, int(tile_bits))


class _BmaInfo(C.Structure):
    _fields_ = [("nvars", C.c_int32), ("tile_bits", C.c_int32), ("passes", C.c_int32), ("levels", C.c_int32),
                ("prior", C.c_int32), ("pad", C.c_int32), ("families_scored", C.c_int64), ("batches", C.c_int64),
                ("lattice_bytes", C.c_int64), ("log_z", C.c_double), ("b_full", C.c_double),
                ("score_kernel_ms", C.c_double), ("alpha_kernel_ms", C.c_double), ("level_kernel_ms", C.c_double),
                ("gamma_kernel_ms", C.c_double), ("q_kernel_ms", C.c_double), ("score_wall_ms", C.c_double),
                ("upload_wall_ms", C.c_double), ("alpha_wall_ms", C.c_double), ("level_wall_ms", C.c_double),
                ("gamma_wall_ms", C.c_double), ("q_wall_ms", C.c_double), ("wall_ms", C.c_double)]


def _lse_exp(x):
    """fbn_bma_lse_exp, a testing entry: e^x for x <= 0 as the arc-posterior lattices evaluate it.  Host only."""
    y = C.c_double()
    lib.fbn_bma_lse_exp(float(x), C.byref(y))
    return y.value


def _lse(a, b):
    """fbn_bma_lse, a testing entry: ln(e^a + e^b) as the arc-posterior lattices evaluate it.  Host only."""
    y = C.c_double()
    lib.fbn_bma_lse(float(a), float(b), C.byref(y))
    return y.value


class ArcPosterior(_ScoredLearner):
    """Exact arc posteriors for up to 26 variables: P(u -> v | data) for every arc by Bayesian model averaging
    over all DAGs, the sum-product counterpart of ExactSearch's dynamic programme (fbn_bma_run; Koivisto & Sood
    2004; no reference counterpart).  score, max_parents, max_family_cells, allowed and learn(source, host) are
    ExactSearch's.  Under "bde" / ("bde", iss) / "k2" the local score is a log marginal likelihood and the
    result a true posterior; under "bic" / "aic" it is the usual exp(score) approximation of one.

    The structure prior is order-modular: uniform over the pairs (linear order, DAG consistent with it), so a
    DAG weighs in proportion to its number of linear extensions -- the price of the exact algorithm and standard
    for it.  prior: "uniform" (0) adds nothing per family, "indegree" (1) adds -ln C(n - 1, |parents|).

    Results: .arc_prob [n][n] (arc_prob[u][v] = P(u -> v | data), zero diagonal), .skeleton_prob (arc_prob +
    its transpose), .log_z (the log normaliser F[V]), .b_full (B[V], equal to it up to rounding), .q_empty [n]
    (each 1 up to rounding), .info (the phase record: passes, kernel and wall ms per phase).  host=True runs the
    host twin (fbn_bma_run_host) on a Dataset, bit-identical, without a device.  `.ci` is shared as
    HillClimbing.ci is."""

    PRIORS = {"uniform": 0, "indegree": 1}

    def __init__(self, score="bde", max_parents=None, max_family_cells=0, allowed=None, prior=0, device=0):
        super().__init__(score, max_parents, max_family_cells, allowed, device)
        self.prior = self.PRIORS.get(prior, prior)

    def learn(self, source, host=False):
        r = self._call("bma", source, host, int(self.prior), self._BD)
        try:
            info = _BmaInfo()
            lib.fbn_bma_result_info(r, C.byref(info))
            n = info.nvars
            self.arc_prob, self.q_empty = np.zeros((n, n)), np.zeros(n)
            lib.fbn_bma_result_arcs(r, _p(self.arc_prob), _p(self.q_empty))
        finally:
            lib.fbn_bma_result_destroy(r)
        self.log_z, self.b_full = info.log_z, info.b_full
        self.skeleton_prob = self.arc_prob + self.arc_prob.T
        self.info = {k: getattr(info, k) for k, _ in _BmaInfo._fields_ if k != "pad"}
        return self

    @staticmethod
    def set_tuning(ci, tile_bits=0):
        """fbn_bma_set_tuning on a context: bits per pass of the three transforms; 0 = default."""
        lib.fbn_bma_set_tuning(ci._h, int(tile_bits))


class _OmcmcOptions(C.Structure):
    _fields_ = [("chains", C.c_int32), ("samples", C.c_int32), ("burn_in", C.c_int64), ("thin", C.c_int64),
                ("seed", C.c_uint64), ("chain_offset", C.c_int64), ("max_families", C.c_int64)]


class _OmcmcInfo(C.Structure):
    _fields_ = [("nvars", C.c_int32), ("prior", C.c_int32), ("chains", C.c_int32), ("samples", C.c_int32),
                ("chains_per_group", C.c_int32), ("launches", C.c_int32), ("burn_in", C.c_int64), ("thin", C.c_int64),
                ("steps", C.c_int64), ("steps_per_launch", C.c_int64), ("families", C.c_int64),
                ("family_bytes", C.c_int64), ("families_scored", C.c_int64), ("batches", C.c_int64),
                ("score_kernel_ms", C.c_double), ("chain_kernel_ms", C.c_double), ("score_wall_ms", C.c_double),
                ("upload_wall_ms", C.c_double), ("chain_wall_ms", C.c_double), ("wall_ms", C.c_double)]


class OrderMCMC(_ScoredLearner):
    """Arc posteriors for up to 64 variables by MCMC over node orders (fbn_omcmc_run; Friedman & Koller 2003; no
    reference counterpart): Metropolis-Hastings chains whose stationary arc probabilities are ArcPosterior's
    arc_prob, under the same scores, candidates (max_parents, max_family_cells, allowed) and order-modular prior
    ("uniform" / "indegree").  One chain per wave on the device; `chains` independent chains start from seeded
    random orders, discard burn_in steps and then take `samples` samples `thin` steps apart.  chain_offset numbers
    the chains within the seed's stream, so two runs of 35 chains at offsets 0 and 35 are one run of 70;
    max_families caps the family lists (0: 2^26 entries).

    learn(source, host=False) is ArcPosterior's (`.ci` is shared the same way; host=True runs the host twin,
    bit-identical, without a device).  Results: .arc_prob [n][n], .skeleton_prob, .chain_arc_prob [chains][n][n]
    (the chains are independent: their spread gives .arc_se, the standard error of arc_prob), .orders [chains][n]
    (the last orders), .log_score [chains][samples] (the order's log score L at every sample), .accept_rate
    [chains], .info.  order_terms(orders, source, host) is a testing entry: the sampler's scan on given orders."""

    PRIORS = ArcPosterior.PRIORS

    def __init__(self, score="bde", max_parents=3, max_family_cells=0, allowed=None, prior=0, chains=64, burn_in=2000,
                 thin=20, samples=200, seed=0, device=0, chain_offset=0, max_families=0):
        super().__init__(score, max_parents, max_family_cells, allowed, device)
        self.prior = self.PRIORS.get(prior, prior)
        self.chains, self.burn_in, self.thin, self.samples, self.seed = chains, burn_in, thin, samples, seed
        self.chain_offset, self.max_families = chain_offset, max_families

    def learn(self, source, host=False):
        m = _OmcmcOptions(int(self.chains), int(self.samples), int(self.burn_in), int(self.thin), int(self.seed),
                          int(self.chain_offset), int(self.max_families))
        r = self._call("omcmc", source, host, int(self.prior), self._BD, C.byref(m))
        try:
            info = _OmcmcInfo()
            lib.fbn_omcmc_result_info(r, C.byref(info))
            n, ch = info.nvars, info.chains
            self.arc_prob, self.chain_arc_prob = np.zeros((n, n)), np.zeros((ch, n, n))
            self.orders, self.log_score = np.zeros((ch, n), np.int32), np.zeros((ch, info.samples))
            accepted = np.zeros(ch, np.int64)
            lib.fbn_omcmc_result_arcs(r, _p(self.arc_prob), _p(self.chain_arc_prob), _p(self.orders), _p(self.log_score),
                                      _p(accepted))
        finally:
            lib.fbn_omcmc_result_destroy(r)
        self.accepted = accepted
        self.accept_rate = accepted / float(info.steps)
        self.skeleton_prob = self.arc_prob + self.arc_prob.T
        self.arc_se = self.chain_arc_prob.std(axis=0, ddof=1) / np.sqrt(ch) if ch > 1 else np.full((n, n), np.inf)
        self.info = {k: getattr(info, k) for k, _ in _OmcmcInfo._fields_}
        return self

    def order_terms(self, orders, source=None, host=False):
        """fbn_omcmc_order_terms(_host): (term [k][n], arcs [k][n][n]) of the orders [k][n] -- term[i][v] the log-sum-exp
        of v's candidate parent sets within its predecessors in order i, arcs[i][u][v] = P(u -> v | order i).  source
        as learn's; None: the context of the last learn."""
        od = np.ascontiguousarray(orders, np.int32)
        k, n = od.shape
        term, arcs = np.zeros((k, n)), np.zeros((k, n, n))
        bd = _bd_score(self.score_name)
        lead, nvars, nsamples = self._source(source, host)
        o, keep = self._options(nvars, nsamples)
        getattr(lib, "fbn_omcmc_order_terms" + ("_host" if host else ""))(
            *lead, C.byref(o), int(self.prior), C.byref(bd) if bd is not None else None, int(self.max_families), _p(od), k,
            _p(term), _p(arcs))
        del keep
        return term, arcs

    @staticmethod
    def set_tuning(ci, chains_per_group=0, steps_per_launch=0):
        """fbn_omcmc_set_tuning on a context: chains (waves) per workgroup, 1 .. 16, and steps per kernel launch;
        0 = default.  The same bits either way."""
        lib.fbn_omcmc_set_tuning(ci._h, int(chains_per_group), int(steps_per_launch))


def score_marginals(network, marginals, golden):
    """fbn_score_marginals: (mse_sum, hd_sum) of marginals [n][sum_dom] against a golden table, as
    JunctionTree.score computes them, from the network alone (no plan)."""
    m = np.ascontiguousarray(marginals, np.float64)
    g = np.ascontiguousarray(golden, np.float64)
    mse, hd = C.c_double(), C.c_double()
    lib.fbn_score_marginals(network._h, _p(m), _p(g), m.shape[0], C.byref(mse), C.byref(hd))
    return mse.value, hd.value


class _CaseInference:
    """What the approximate case-inference classes share: the buffers of infer and debug_samples, the
    eps argument and EvaluateAccuracy.  The class sets self.network and self.sum_dom and defines infer."""

    def _outputs(self, evidence, marginals, k):
        """(evidence int8, ncases, labels, marginals or None, stats [ncases][k]) of one infer call."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        labels = np.zeros(n, np.int32)
        marg = np.zeros((n, self.sum_dom), np.float64) if marginals else None
        return ev, n, labels, marg, np.zeros((n, k), np.float64)

    def _debug_outputs(self, evidence, draws):
        """(evidence int8, ncases, values, mantissas, exponents) for `draws` samples per case."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        tot = n * draws
        return (ev, n, np.zeros((self.network.num_nodes, tot), np.uint8), np.zeros(tot, np.float64),
                np.zeros(tot, np.int32))

    @staticmethod
    def _eps_arg(eps):
        """The C entries' eps: None -> -1.0 (they read a negative eps as "the defaults")."""
        if eps is None:
            return -1.0
        if float(eps) < 0.0:
            err = FastBNError(f"eps {eps!r}: in [0, 1), or None for the defaults")
            err.code = -1  # FBN_ERR_ARG
            raise err
        return float(eps)

    def EvaluateAccuracy(self, evidence, ground_truths, golden=None):
        """Accuracy of the query-variable arg-max (+ average MSE/HD vs golden if given)."""
        labels, marg = self.infer(evidence)
        acc = float(np.mean(labels == np.asarray(ground_truths)))
        if golden is None:
            return acc
        mse, hd = score_marginals(self.network, marg, golden)
        return acc, mse / len(labels), hd / len(labels)


class Sampler(_Handle):
    """The sampling engine of one network on one device (fbn_sampler).  device < 0: the host path,
    the same algorithm on CPU threads (bit-identical results)."""

    _destroy = "fbn_sampler_destroy"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        lib.fbn_sampler_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def forward_sample(self, n, seed):
        """n complete cases, uint8 [V][n]; = Network.forward_sample(n, seed) = synth.forward_sample."""
        cols = np.empty((self.network.num_nodes, int(n)), np.uint8)
        lib.fbn_sample_forward(self._h, int(n), int(seed), _p(cols))
        return cols

    def forward_sample_device(self, d_cols_ptr, n, seed, stream_ptr=None):
        """The same into a device buffer uint8 [V][n] (e.g. IndependenceTest.from_device's input);
        asynchronous on the stream."""
        lib.fbn_sample_forward_device(self._h, int(n), int(seed), C.c_void_p(d_cols_ptr), stream_ptr)

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_sampler_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class LikelihoodWeighting(_CaseInference, Sampler):
    """Sampling inference, mirroring JunctionTree: likelihood weighting (method="lw", the reference's
    -a 5) or probabilistic logic sampling ("pls", -a 4) with num_samples samples per case (-q).
    Works on any DAG, a disconnected learned network included."""

    _METHODS = {"lw": 0, "pls": 1}

    def __init__(self, network, num_samples=10000, seed=0, device=0, method="lw"):
        if method not in self._METHODS:
            raise FastBNError(f"method {method!r}: 'lw' or 'pls'")
        super().__init__(network, device)
        self.num_samples, self.seed, self.method = int(num_samples), int(seed), self._METHODS[method]
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess) per case.  case_offset: the global index of the first case
        (a batch split over calls gives the bits of the whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 2)
        lib.fbn_lw_run(self._h, self.method, _p(ev), n, self.num_samples, self.seed, int(case_offset), _p(labels),
                       _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_lw_run_device(self._h, self.method, C.c_void_p(d_evidence_ptr), int(ncases), self.num_samples,
                              self.seed, int(case_offset), C.c_void_p(d_labels_ptr),
                              C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                              C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """The samples behind infer(evidence): (values uint8 [V][ncases * S], mantissas fp64,
        exponents int32 [ncases * S]); sample s of case c at c * S + s."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.num_samples)
        lib.fbn_lw_debug_samples(self._h, self.method, _p(ev), n, self.num_samples, self.seed, int(case_offset),
                                 _p(vals), _p(m), _p(e))
        return vals, m, e


class LoopyBeliefPropagation(_CaseInference, _Handle):
    """Loopy belief propagation (fbn_lbp; the reference's -a 7 stub, src/main.cpp:136-147), mirroring
    JunctionTree: `iterations` flooding sweeps (the reference's propagation length, -d), stopping
    early once an iteration's residual is <= tol; `damping` in [0, 1) on the factor -> variable
    messages.  Exact on forests / polytrees, an approximation on loopy graphs.  Works on any DAG, a
    disconnected learned network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_lbp_destroy"

    def __init__(self, network, iterations=2, tol=0.0, damping=0.0, device=0):
        self.network = network
        self.iterations, self.tol, self.damping = int(iterations), float(tol), float(damping)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_lbp_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(edges, msg_doubles, lds_bytes, path): path 0 = messages in LDS, 1 = global workspace."""
        e, m, b, p = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_lbp_info(self._h, C.byref(e), C.byref(m), C.byref(b), C.byref(p))
        return {"edges": e.value, "msg_doubles": m.value, "lds_bytes": b.value, "path": p.value}

    def infer(self, evidence, marginals=True):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (iterations used, last residual) per case."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 2)
        lib.fbn_lbp_run(self._h, _p(ev), n, self.iterations, self.tol, self.damping, _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].astype(np.int32), st[:, 1].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr, d_stats_ptr=None, stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_lbp_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), self.iterations, self.tol,
                               self.damping, C.c_void_p(d_labels_ptr), C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                               C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_messages(self, evidence, iterations):
        """Both message arrays [ncases][2][msg_doubles] (factor -> variable, then variable ->
        factor) after exactly `iterations` iterations."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        out = np.zeros((n, 2, self.info()["msg_doubles"]), np.float64)
        lib.fbn_lbp_debug_messages(self._h, _p(ev), n, int(iterations), self.damping, _p(out))
        return out

    def set_tuning(self, lds_bytes_max=0, max_groups=0):
        """fbn_lbp_set_tuning: lds_bytes_max < 0 forces the global message workspace; max_groups caps
        the persistent grid.  0 = default.  Results do not change."""
        lib.fbn_lbp_set_tuning(self._h, int(lds_bytes_max), int(max_groups))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_lbp_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class EPISBN(_CaseInference, _Handle):
    """EPIS-BN (fbn_epis; the reference's -a 6 stub, src/main.cpp:123-134), mirroring JunctionTree:
    `iterations` sweeps of loopy belief propagation (tol, damping as LoopyBeliefPropagation), then
    importance sampling with num_samples samples per case (-q) from each CPT row times the lambda
    message LBP left on the variable.  eps: the cutoff in [0, 1), None = the defaults by state count.
    iterations=0 is likelihood weighting's draws.  Unbiased; works on any DAG, a disconnected learned
    network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_epis_destroy"

    def __init__(self, network, num_samples=10000, iterations=20, tol=0.0, damping=0.0, eps=None, seed=0, device=0):
        self.network = network
        self.num_samples, self.seed = int(num_samples), int(seed)
        self.iterations, self.tol, self.damping = int(iterations), float(tol), float(damping)
        self.eps = self._eps_arg(eps)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_epis_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def _run_args(self, n, case_offset):
        return (n, self.num_samples, self.seed, int(case_offset), self.iterations, self.tol, self.damping, self.eps)

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess, LBP iterations used, LBP residual) per case.  case_offset: the
        global index of the first case (a batch split over calls gives the bits of the whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 4)
        lib.fbn_epis_run(self._h, _p(ev), *self._run_args(n, case_offset), _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy(), st[:, 2].astype(np.int32), st[:, 3].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr=None, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (two launches, asynchronous on the stream after the evidence check);
        d_stats [ncases][4]."""
        lib.fbn_epis_run_device(self._h, C.c_void_p(d_evidence_ptr), *self._run_args(int(ncases), case_offset),
                                C.c_void_p(d_labels_ptr), C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                                C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """The samples behind infer(evidence): (values uint8 [V][ncases * S], mantissas fp64, exponents
        int32 [ncases * S], lambda rows fp64 [ncases][sum_dom]); sample s of case c at c * S + s."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.num_samples)
        lam = np.zeros((n, self.sum_dom), np.float64)
        lib.fbn_epis_debug_samples(self._h, _p(ev), *self._run_args(n, case_offset), _p(vals), _p(m), _p(e), _p(lam))
        return vals, m, e, lam

    def set_tuning(self, lds_bytes_max=0):
        """fbn_epis_set_tuning: lds_bytes_max < 0 reads the lambda rows from global memory instead of
        LDS; 0 = default.  Results do not change."""
        lib.fbn_epis_set_tuning(self._h, int(lds_bytes_max))

    def info(self):
        """dict(lds_bytes, path): path 0 = the lambda row in LDS, 1 = in global memory."""
        b, p = C.c_int64(), C.c_int()
        lib.fbn_epis_info(self._h, C.byref(b), C.byref(p))
        return {"lds_bytes": b.value, "path": p.value}

    def last_kernel_ms(self):
        """(LBP kernel ms, sampling kernel ms) of the last run."""
        a, b = C.c_float(), C.c_float()
        lib.fbn_epis_last_kernel_ms(self._h, C.byref(a), C.byref(b))
        return a.value, b.value


class AISBN(_CaseInference, _Handle):
    """AIS-BN (fbn_ais, method 0; the reference's -a 10 stub, src/main.cpp:175-186), mirroring EPISBN:
    max_updates (-m) learning stages of `interval` (-l) samples, each followed by an update of the
    importance CPT of the evidence's unobserved ancestors from the stage's weighted family counts,
    then num_samples (-q) counted samples.  eps: the cutoff in [0, 1), None = the defaults by state
    count.  max_updates=0 is likelihood weighting's draws.  Unbiased; needs no LBP; works on any DAG,
    a disconnected learned network included.  device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_ais_destroy"
    _method = 0

    def __init__(self, network, num_samples=10000, max_updates=10, interval=2500, eps=None, seed=0, device=0):
        self.network = network
        self.num_samples, self.seed = int(num_samples), int(seed)
        self.max_updates, self.interval = int(max_updates), int(interval)
        self.eps = self._eps_arg(eps)
        self.sum_dom = int(np.sum(network.dims))
        self.stats = None
        h = C.c_void_p()
        lib.fbn_ais_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    @property
    def draws_per_case(self):
        """T: every draw of a case, the learning stages included."""
        if self._method == 0:
            return self.max_updates * self.interval + self.num_samples
        return self.num_samples

    def _run_args(self, n, case_offset):
        return (n, self.num_samples, self.max_updates, self.interval, self.seed, int(case_offset), self.eps)

    def infer(self, evidence, marginals=True, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None);
        self.stats = (log_evidence, ess, updates applied, ess / n of the first stage) per case.
        case_offset: the global index of the first case (a batch split over calls gives the bits of the
        whole batch)."""
        ev, n, labels, marg, st = self._outputs(evidence, marginals, 4)
        lib.fbn_ais_run(self._h, self._method, _p(ev), *self._run_args(n, case_offset), _p(labels), _p(marg), _p(st))
        self.stats = (st[:, 0].copy(), st[:, 1].copy(), st[:, 2].astype(np.int32), st[:, 3].copy())
        return labels, marg

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr=None, d_stats_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (one launch, asynchronous on the stream after the evidence check);
        d_stats [ncases][4]."""
        lib.fbn_ais_run_device(self._h, self._method, C.c_void_p(d_evidence_ptr),
                               *self._run_args(int(ncases), case_offset), C.c_void_p(d_labels_ptr),
                               C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                               C.c_void_p(d_stats_ptr) if d_stats_ptr else None, stream_ptr)

    def debug_samples(self, evidence, case_offset=0):
        """Every draw behind infer(evidence): (values uint8 [V][ncases * T], mantissas fp64, exponents
        int32 [ncases * T], the importance CPT after the last update fp64 [ncases][cells]); draw t of
        case c at c * T + t, T = draws_per_case."""
        ev, n, vals, m, e = self._debug_outputs(evidence, self.draws_per_case)
        icpt = np.zeros((n, self.info()["state_bytes"] // 16), np.float64)
        lib.fbn_ais_debug_samples(self._h, self._method, _p(ev), *self._run_args(n, case_offset), _p(vals), _p(m), _p(e),
                                  _p(icpt))
        return vals, m, e, icpt

    def set_tuning(self, lds_bytes_max=0, max_workgroups=0):
        """fbn_ais_set_tuning: lds_bytes_max < 0 keeps the importance CPT and the counts in a global
        workspace instead of LDS; max_workgroups caps the persistent grid.  0 = default.  Results do not
        change."""
        lib.fbn_ais_set_tuning(self._h, int(lds_bytes_max), int(max_workgroups))

    def info(self, ncases=1):
        """dict(lds_bytes, state_bytes, path, grid): path 0 = the state in LDS, 1 = in global memory;
        grid = the workgroups a run of ncases cases launches."""
        b, sb, p, g = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        lib.fbn_ais_info(self._h, int(ncases), C.byref(b), C.byref(sb), C.byref(p), C.byref(g))
        return {"lds_bytes": b.value, "state_bytes": sb.value, "path": p.value, "grid": g.value}

    def eta(self):
        """The learning rates eta[0 .. max_updates) the runs use (fbn_ais_eta)."""
        out = np.zeros(max(self.max_updates, 1), np.float64)
        lib.fbn_ais_eta(self._method, self.max_updates, _p(out))
        return out[:self.max_updates]

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_ais_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class SelfImportanceSampling(AISBN):
    """Self-importance sampling (fbn_ais, method 1; the reference's -a 8 stub, src/main.cpp:149-160):
    all num_samples (-q) samples are counted; after each full block of `interval` (-l) samples, while
    samples remain and at most max_updates (-m) times, the importance CPT rows of the evidence's
    unobserved ancestors are replaced by the cumulative weighted frequencies.  It relies on the
    cutoff's floor for support, so eps=0 is refused.  Otherwise as AISBN."""

    _method = 1


class MostProbableExplanation(_Handle):
    """Most probable explanation (fbn_mpe): the complete assignment x* = argmax_x P(x, e) that agrees with
    the evidence, and log P(x*, e) -- exact, by max-product message passing with a back-trace on the
    junction forest, so it takes any DAG.  The value is kept as a mantissa and a binary exponent and
    does not underflow on networks of thousands of variables.  The reference has no counterpart.
    device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_mpe_destroy"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        lib.fbn_mpe_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(cliques, entries, store_rows, components): store_rows = rows of one case's store."""
        c, e, r, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_mpe_info(self._h, C.byref(c), C.byref(e), C.byref(r), C.byref(k))
        return {"cliques": c.value, "entries": e.value, "store_rows": r.value, "components": k.value}

    def value_parts(self, evidence):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (assignment int8 [ncases][num_nodes],
        value fp64 [ncases][2] = (m, ex) with P(x*, e) = m * 2^ex, m in [0.5, 1)).  A case whose value
        underflows inside a clique (m would be 0) raises FastBNError (FBN_ERR_LIMIT) naming it."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        assign = np.zeros((n, self.network.num_nodes), np.int8)
        value = np.zeros((n, 2), np.float64)
        lib.fbn_mpe_run(self._h, _p(ev), n, _p(assign), _p(value))
        return assign, value

    def infer(self, evidence):
        """-> (assignment int8 [ncases][num_nodes], log_p fp64 [ncases] = log P(x*, e))."""
        assign, value = self.value_parts(evidence)
        return assign, np.log(value[:, 0]) + value[:, 1] * np.log(2.0)

    def run_device(self, d_evidence_ptr, ncases, d_assignment_ptr, d_value_ptr, stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_mpe_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), C.c_void_p(d_assignment_ptr),
                               C.c_void_p(d_value_ptr), stream_ptr)

    def debug_messages(self, evidence):
        """(messages fp64 [ncases][sum of separator entries], exponents int32 [ncases][separators]) as
        Collect leaves them."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        i = self.info()
        nsep = i["cliques"] - i["components"]
        msg = np.zeros((n, i["store_rows"] - nsep - i["cliques"]), np.float64)
        exps = np.zeros((n, nsep), np.int32)
        lib.fbn_mpe_debug_messages(self._h, _p(ev), n, _p(msg), _p(exps))
        return msg, exps

    def set_tuning(self, max_workgroups=0, store_bytes_max=0):
        """fbn_mpe_set_tuning: max_workgroups caps the persistent grid, store_bytes_max the message store
        of all waves together.  0 = default.  Results do not change."""
        lib.fbn_mpe_set_tuning(self._h, int(max_workgroups), int(store_bytes_max))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_mpe_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class ExpectationMaximization(_Handle):
    """Parameter learning from incomplete data (fbn_em): expectation-maximisation over the junction forest
    of `network`, whose structure is kept and whose probabilities are the starting parameters.  Data rows
    are int8 [ncases][num_nodes], -1 = missing.  The E-step runs exact junction-tree inference per row (one
    row per GPU lane) and sums the family posteriors; the M-step is (N + pseudo_count) / (T + pseudo_count
    * states).  The reference has no counterpart.  device < 0: the host twin (the same per-case bytes)."""

    _destroy = "fbn_em_destroy"

    def __init__(self, network, pseudo_count=1.0, device=0):
        if not pseudo_count > 0:
            err = FastBNError(f"ExpectationMaximization: the pseudo-count must be > 0 (got {pseudo_count})")
            err.code = -1
            raise err
        self.network_start = network
        self.pseudo_count = float(pseudo_count)
        self.num_nodes = network.num_nodes
        self.dims = network.dims.copy()
        self._npc = [network.node_probs(v)[1].shape[1] for v in range(self.num_nodes)]
        h = C.c_void_p()
        lib.fbn_em_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(cliques, entries, store_rows, cells, components)."""
        c, e, r, n, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_em_info(self._h, C.byref(c), C.byref(e), C.byref(r), C.byref(n), C.byref(k))
        return {"cliques": c.value, "entries": e.value, "store_rows": r.value, "cells": n.value, "components": k.value}

    def _split(self, flat):
        """the flat cell array as one [dims[v], parent configs] view per node"""
        out, off = [], 0
        for v in range(self.num_nodes):
            n = int(self.dims[v]) * self._npc[v]
            out.append(flat[off:off + n].reshape(int(self.dims[v]), self._npc[v]))
            off += n
        return out

    def estep_flat(self, data):
        """-> (counts fp64 [cells], value fp64 [ncases][2] = (m, ex), P(e) = m * 2^ex)."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        n = d.shape[0]
        counts = np.zeros(self.info()["cells"], np.float64)
        value = np.zeros((n, 2), np.float64)
        lib.fbn_em_estep(self._h, _p(d), n, _p(counts), _p(value))
        return counts, value

    def estep(self, data):
        """One E-step at the current parameters -> (counts: one [dims[v], parent configs] array per node,
        value [ncases][2])."""
        counts, value = self.estep_flat(data)
        return self._split(counts), value

    def estep_device(self, d_data_ptr, ncases, d_counts_ptr, d_value_ptr, stream_ptr=None):
        """Device-resident E-step (asynchronous on the stream after the data check)."""
        lib.fbn_em_estep_device(self._h, C.c_void_p(d_data_ptr), int(ncases), C.c_void_p(d_counts_ptr),
                                C.c_void_p(d_value_ptr) if d_value_ptr else None, stream_ptr)

    def fit(self, data, max_iters=50, tol=1e-6):
        """Iterate E-step and M-step -> objective fp64 [iters_done][2] = (log-likelihood, Q) at the
        parameters each iteration's E-step ran with.  tol = 0 never stops early."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        obj = np.zeros((max(int(max_iters), 1), 2), np.float64)
        done = C.c_int()
        lib.fbn_em_run(self._h, _p(d), d.shape[0], int(max_iters), float(tol), self.pseudo_count, _p(obj), C.byref(done))
        return obj[:done.value].copy()

    def network(self):
        """The current parameters as a probability network."""
        h = C.c_void_p()
        lib.fbn_em_network(self._h, C.byref(h))
        return Network(_handle=h)

    def set_parameters(self, net):
        """Take net's probabilities (same structure, else an error)."""
        lib.fbn_em_set_parameters(self._h, net._h)

    def debug_posteriors(self, data):
        """The per-case family posteriors fp64 [ncases][cells]."""
        d = np.ascontiguousarray(data, dtype=np.int8)
        post = np.zeros((d.shape[0], self.info()["cells"]), np.float64)
        lib.fbn_em_debug_posteriors(self._h, _p(d), d.shape[0], _p(post))
        return post

    def log_likelihood(self, data):
        """log P(e) per case fp64 [ncases] at the current parameters."""
        _, value = self.estep_flat(data)
        return np.log(value[:, 0]) + value[:, 1] * np.log(2.0)

    def set_tuning(self, max_workgroups=0, store_bytes_max=0):
        """fbn_em_set_tuning, as MostProbableExplanation.set_tuning.  Per-case results do not change."""
        lib.fbn_em_set_tuning(self._h, int(max_workgroups), int(store_bytes_max))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_em_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class PosteriorSampler(_Handle):
    """Exact posterior sampling (fbn_psample): complete assignments distributed as P(x | e) and log P(e), by
    a sum-product Collect and a sampled top-down trace on the junction forest, so it takes any DAG.  Every
    draw is independent and weighs 1, however unlikely the evidence.  A sample depends on (seed, case_offset
    + case, sample index, draws) alone: never on the batch, its split, the grid or the device; changing
    `draws` changes every sample (the stream position uses it).  The reference has no counterpart.
    device < 0: the host twin (bit-identical results)."""

    _destroy = "fbn_psample_destroy"

    def __init__(self, network, device=0):
        self.network = network
        h = C.c_void_p()
        lib.fbn_psample_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def info(self):
        """dict(cliques, entries, store_rows, components): store_rows = rows of one wave's store."""
        c, e, r, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        lib.fbn_psample_info(self._h, C.byref(c), C.byref(e), C.byref(r), C.byref(k))
        return {"cliques": c.value, "entries": e.value, "store_rows": r.value, "components": k.value}

    def value_parts(self, evidence, draws=1, seed=0, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (samples int8 [ncases][draws][num_nodes],
        value fp64 [ncases][2] = (m, ex) with P(e) = m * 2^ex, m in [0.5, 1)).  A case of probability 0
        raises FastBNError (FBN_ERR_LIMIT) naming it."""
        ev = np.ascontiguousarray(evidence, dtype=np.int8)
        n = ev.shape[0]
        samples = np.zeros((n, max(int(draws), 0), self.network.num_nodes), np.int8)
        value = np.zeros((n, 2), np.float64)
        lib.fbn_psample_run(self._h, _p(ev), n, int(draws), int(seed), int(case_offset), _p(samples), _p(value))
        return samples, value

    def sample(self, evidence, draws=1, seed=0, case_offset=0):
        """-> (samples int8 [ncases][draws][num_nodes], log_p fp64 [ncases] = log P(e))."""
        samples, value = self.value_parts(evidence, draws, seed, case_offset)
        return samples, np.log(value[:, 0]) + value[:, 1] * np.log(2.0)

    def run_device(self, d_evidence_ptr, ncases, draws, d_samples_ptr, d_value_ptr, seed=0, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check)."""
        lib.fbn_psample_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), int(draws), int(seed),
                                   int(case_offset), C.c_void_p(d_samples_ptr), C.c_void_p(d_value_ptr), stream_ptr)

    def set_tuning(self, max_workgroups=0, store_bytes_max=0, sample_chunk=0):
        """fbn_psample_set_tuning: the grid cap and the store budget as MostProbableExplanation.set_tuning;
        sample_chunk = draws of a case that share one Collect.  0 = default.  Results do not change."""
        lib.fbn_psample_set_tuning(self._h, int(max_workgroups), int(store_bytes_max), int(sample_chunk))

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_psample_last_kernel_ms(self._h, C.byref(ms))
        return ms.value


class GibbsSampling(_CaseInference, _Handle):
    """Gibbs sampling (fbn_gibbs, -a 16), mirroring the samplers: per evidence case `chains` independent
    chains, each a forward start with the evidence clamped, burn_in discarded sweeps and `sweeps` counted
    ones over the unobserved variables; the marginals are the Rao-Blackwell average of the conditionals the
    draws were made from.  Nothing is weighed, so unlikely evidence costs nothing, and only the tables of a
    variable and its children are read, so any DAG is taken.  Not ergodic where zero table entries
    disconnect the state space (no network built here has one).  A case's result depends on (seed, global
    case index, chains, burn_in, sweeps) alone.  The reference has no counterpart.  device < 0: the host
    twin (bit-identical results)."""

    _destroy = "fbn_gibbs_destroy"

    def __init__(self, network, chains=64, sweeps=256, burn_in=64, seed=0, device=0):
        self.network = network
        self.chains, self.sweeps, self.burn_in, self.seed = int(chains), int(sweeps), int(burn_in), int(seed)
        self.sum_dom = int(np.sum(network.dims))
        h = C.c_void_p()
        lib.fbn_gibbs_create(network._h, int(device), C.byref(h))
        self._h = h
        _register(self)

    def infer(self, evidence, marginals=True, states=False, case_offset=0):
        """evidence [ncases][num_nodes] int8 (-1 unobserved) -> (labels, marginals or None), and with
        states=True a third item: the chains' last assignments int8 [ncases][chains][num_nodes], `chains`
        draws per case from approximately P(x | e).  case_offset: the global index of the first case (a
        batch split over calls gives the bits of the whole batch)."""
        ev, n, labels, marg, _ = self._outputs(evidence, marginals, 0)
        st = np.zeros((n, max(self.chains, 0), self.network.num_nodes), np.int8) if states else None
        lib.fbn_gibbs_run(self._h, _p(ev), n, self.chains, self.burn_in, self.sweeps, self.seed, int(case_offset),
                          _p(labels), _p(marg), _p(st))
        return (labels, marg, st) if states else (labels, marg)

    def run_device(self, d_evidence_ptr, ncases, d_labels_ptr, d_marg_ptr=None, d_states_ptr=None, case_offset=0,
                   stream_ptr=None):
        """Device-resident run (asynchronous on the stream after the evidence check); d_states int8
        [ncases][chains][num_nodes] or None."""
        lib.fbn_gibbs_run_device(self._h, C.c_void_p(d_evidence_ptr), int(ncases), self.chains, self.burn_in,
                                 self.sweeps, self.seed, int(case_offset), C.c_void_p(d_labels_ptr),
                                 C.c_void_p(d_marg_ptr) if d_marg_ptr else None,
                                 C.c_void_p(d_states_ptr) if d_states_ptr else None, stream_ptr)

    def conditionals(self, states):
        """states int8 [n][num_nodes], complete assignments -> fp64 [n][sum_dom]: every variable's normalised
        conditional given all the others, by the function the sweep calls (fbn_gibbs_debug_conditionals)."""
        st = np.ascontiguousarray(states, dtype=np.int8)
        out = np.zeros((st.shape[0], self.sum_dom), np.float64)
        lib.fbn_gibbs_debug_conditionals(self._h, _p(st), st.shape[0], _p(out))
        return out

    def set_tuning(self, lds_bytes_max=0, max_workgroups=0, pc_cache=-1):
        """fbn_gibbs_set_tuning: lds_bytes_max < 0 keeps the accumulators in a global workspace instead of
        LDS; max_workgroups caps the persistent grid; pc_cache 0 / 1 recomputes / caches the children's
        parent configurations (-1: the default).  Results do not change."""
        lib.fbn_gibbs_set_tuning(self._h, int(lds_bytes_max), int(max_workgroups), int(pc_cache))

    def info(self, ncases=1):
        """dict(lds_bytes, path, pc_cache, grid): path 0 = the accumulators in LDS, 1 = in global memory;
        grid = the workgroups a run of ncases cases launches."""
        b, p, k, g = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        lib.fbn_gibbs_info(self._h, int(ncases), max(self.chains, 1), C.byref(b), C.byref(p), C.byref(k), C.byref(g))
        return {"lds_bytes": b.value, "path": p.value, "pc_cache": k.value, "grid": g.value}

    def last_kernel_ms(self):
        ms = C.c_float()
        lib.fbn_gibbs_last_kernel_ms(self._h, C.byref(ms))
        return ms.value
