"""ctypes binding of ``librn_potgnn.so`` (the C ABI declared in ``include/rn_potgnn.h``).

There is no CPU fallback: if the library is missing or a device call fails the caller
gets a ``DeviceError``.
"""
from __future__ import annotations

import ctypes as C
import os

from ramannoodle_amd.exceptions import DeviceError

_LIB_PATH = os.environ.get(
    "RN_POTGNN_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "librn_potgnn.so"))

RN_OK = 0
RN_ERR_INVALID_ARGUMENT = -1
RN_ERR_UNSUPPORTED = -2
RN_ERR_NO_DEVICE = -3
RN_ERR_HIP = -4
RN_ERR_OUT_OF_MEMORY = -5


class Config(C.Structure):
    """``rn_potgnn_config``."""

    _fields_ = [
        ("num_atoms", C.c_int32),
        ("num_edges", C.c_int32),
        ("num_atom_types", C.c_int32),
        ("size_node_embedding", C.c_int32),
        ("size_edge_embedding", C.c_int32),
        ("num_message_passes", C.c_int32),
        ("gauss_coefficient", C.c_double),
        ("max_chunk_structures", C.c_int32),
        ("device", C.c_int32),
    ]


# symbol -> (restype, argtypes); must list every function declared in include/*.h
_P = C.c_void_p
SIGNATURES = {
    "rn_potgnn_radius_graph": (C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_int, _P]),
    "rn_potgnn_config_flags": (C.c_int, [_P]),
    "rn_potgnn_set_stat_reducer": (C.c_int, [_P, _P, _P]),
    "rn_potgnn_train_row_count": (C.c_double, [_P]),
    "rn_potgnn_weight_count": (C.c_size_t, [C.POINTER(Config)]),
    "rn_potgnn_create": (C.c_int, [C.POINTER(Config), _P, _P, _P, _P, _P, C.c_size_t, _P, _P,
                                   C.POINTER(_P)]),
    "rn_potgnn_destroy": (None, [_P]),
    "rn_potgnn_calc_polarizabilities": (C.c_int, [_P, _P, C.c_int64, _P]),
    "rn_potgnn_calc_polarizabilities_f64": (C.c_int, [_P, _P, C.c_int64, _P]),
    "rn_potgnn_calc_polarizabilities_to_device": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "rn_potgnn_calc_polarizabilities_cells": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P]),
    "rn_potgnn_calc_polarizabilities_cells_to_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    "rn_potgnn_forward_cells_device": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, C.c_int]),
    "rn_potgnn_descriptors": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P]),
    "rn_potgnn_device_descriptors": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "rn_potgnn_forward_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_int]),
    "rn_potgnn_forward_device_f64": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int]),
    "rn_potgnn_calc_polarizabilities_async": (C.c_int, [_P, _P, C.c_int64, _P]),
    "rn_potgnn_wait": (C.c_int, [_P]),
    "rn_host_buffer_alloc": (C.c_int, [C.c_size_t, C.c_int, C.POINTER(_P)]),
    "rn_host_buffer_free": (None, [_P]),
    "rn_potgnn_forward": (C.c_int, [_P, _P, C.c_int64, _P]),
    "rn_potgnn_forward_lattices": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rn_potgnn_forward_samples": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    "rn_potgnn_forward_samples_f64": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    "rn_potgnn_raman_tensors": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, _P]),
    "rn_potgnn_alpha_jacobian": (C.c_int, [_P, _P, C.c_int, _P]),
    "rn_potgnn_raman_tensors_analytic": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "rn_potgnn_set_weights": (C.c_int, [_P, _P, C.c_size_t]),
    "rn_potgnn_train_forward": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "rn_potgnn_train_backward": (C.c_int, [_P, _P, _P]),
    "rn_potgnn_set_device_training": (C.c_int, [_P, C.c_int]),
    "rn_potgnn_train_backward_device": (C.c_int, [_P, _P]),
    "rn_potgnn_gradient_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "rn_potgnn_adam_step": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64]),
    "rn_potgnn_get_weights": (C.c_int, [_P, _P, C.c_size_t]),
    "rn_potgnn_train_forward_f64": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "rn_potgnn_train_forward_samples": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P]),
    "rn_potgnn_train_forward_samples_f64": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P]),
    "rn_potgnn_forward_samples_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, C.c_int]),
    "rn_potgnn_train_forward_samples_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P]),
    "rn_potgnn_train_backward_samples_device": (C.c_int, [_P, _P, _P]),
    "rn_potgnn_train_backward_f64": (C.c_int, [_P, _P, _P]),
    "rn_potgnn_forward_vjp_device": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_int, _P, _P, _P]),
    "rn_potgnn_group_increments_device": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_size_t, _P, _P]),
    "rn_potgnn_group_increments_cells_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_size_t, _P,
                                                          _P]),
    "rn_potgnn_partial_raman_tensors": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int, _P]),
    "rn_potgnn_mode_contract_device": (C.c_int, [_P, C.c_int64, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int, C.c_int,
                                                 _P, _P]),
    "rn_potgnn_mode_increments_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int, C.c_int,
                                                   C.c_size_t, _P, _P]),
    "rn_potgnn_train_backward_inputs": (C.c_int, [_P, _P, _P, _P, _P]),
    "rn_potgnn_train_backward_inputs_device": (C.c_int, [_P, _P, _P, _P, _P]),
    "rn_potgnn_num_triplets": (C.c_int64, [_P]),
    "rn_potgnn_debug_triplets": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "rn_potgnn_debug_ps_schedule": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "rn_potgnn_debug_plan": (C.c_int, [C.POINTER(Config), _P, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rn_potgnn_debug_plan_pairs": (C.c_int, [C.POINTER(Config), _P, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rn_potgnn_debug_plan_lds": (C.c_int, [C.POINTER(Config), _P, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rn_potgnn_debug_pack_weights": (C.c_int, [C.POINTER(Config), _P, C.c_size_t, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rn_potgnn_debug_unpack_weights": (C.c_int, [C.POINTER(Config), _P, C.c_size_t, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rn_potgnn_debug_stage": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rn_potgnn_set_profiling": (C.c_int, [_P, C.c_int]),
    "rn_potgnn_kernel_times": (C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int64), C.c_int]),
    "rn_potgnn_last_error": (C.c_char_p, [_P]),
    "rn_potgnn_version": (C.c_char_p, []),
    "rn_md_raman_intensities": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64]),
    "rn_md_raman_intensities_device": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, _P]),
    "rn_md_raman_polarized": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_polarized_device": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64,
                                               _P]),
    "rn_md_raman_partial": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_partial_device": (C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int, C.c_size_t, _P,
                                             C.c_int64, _P]),
    "rn_md_raman_segments": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.c_int64, C.c_int, C.c_int,
                                       C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_segments_device": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P, C.c_int64, C.c_int, C.c_int,
                                              C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_raman_segments_at": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int, C.c_int,
                                          C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_segments_at_device": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int,
                                                 C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_raman_segment_replicates": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                                 C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_segment_replicates_device": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                                        C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_raman_segment_replicates_set_profiling": (C.c_int, [C.c_int]),
    "rn_md_raman_segment_replicates_phase_times": (C.c_int, [_P]),
    "rn_md_raman_partial_segments": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64,
                                               C.c_int, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_partial_segments_device": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P,
                                                      C.c_int64, C.c_int, C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_vdos": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int, C.c_int64, _P, C.c_int64, _P,
                             C.c_int, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_vdos_device": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int, C.c_int64, _P, C.c_int64,
                                    _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_vdos_set_profiling": (C.c_int, [C.c_int]),
    "rn_md_vdos_phase_times": (C.c_int, [_P]),
    "rn_md_mode_vdos": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int64, _P, C.c_int64,
                                  _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_mode_vdos_device": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int64, _P,
                                         C.c_int64, _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_mode_vdos_set_profiling": (C.c_int, [C.c_int]),
    "rn_md_mode_vdos_phase_times": (C.c_int, [_P]),
    "rn_md_raman_modes": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int, C.c_int,
                                    C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_modes_device": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int,
                                           C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_raman_modes_set_profiling": (C.c_int, [C.c_int]),
    "rn_md_raman_modes_phase_times": (C.c_int, [_P]),
    "rn_md_raman_mode_matrix": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                          C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64]),
    "rn_md_raman_mode_matrix_device": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                                 C.c_int64, C.c_int, C.c_size_t, _P, C.c_int64, _P]),
    "rn_md_raman_mode_matrix_set_profiling": (C.c_int, [C.c_int]),
    "rn_md_raman_mode_matrix_phase_times": (C.c_int, [_P]),
    "rn_md_raman_mode_matrix_response": (C.c_int, [C.c_int64, _P, C.c_int64, C.c_int64, C.c_double, _P]),
    # include/rn_ingest.h (host-only trajectory reader)
    "rn_xdatcar_open": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "rn_xdatcar_close": (None, [_P]),
    "rn_xdatcar_info": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32)]),
    "rn_xdatcar_species": (C.c_int, [_P, C.c_int32, C.c_char_p, C.POINTER(C.c_int32)]),
    "rn_xdatcar_read": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, C.c_int]),
    "rn_xdatcar_variable_cell": (C.c_int, [_P]),
    "rn_xdatcar_read_lattices": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "rn_xdatcar_last_error": (C.c_char_p, [_P]),
    "rn_vasprun_open": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "rn_vasprun_close": (None, [_P]),
    "rn_vasprun_info": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "rn_vasprun_read": (C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_int]),
    "rn_vasprun_timestep": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "rn_vasprun_initial_num_atoms": (C.c_int64, [_P]),
    "rn_vasprun_initial_structure": (C.c_int, [_P, C.POINTER(C.c_int32), _P, _P, C.c_int64, _P, C.c_int64]),
    "rn_vasprun_last_error": (C.c_char_p, [_P]),
}

# include/rn_interp.h (the interpolation model; a table of its own: SIGNATURES is the rn_potgnn / rn_md / ingest ABI)
INTERP_SIGNATURES = {
    "rn_interp_create": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int, C.POINTER(_P)]),
    "rn_interp_destroy": (None, [_P]),
    "rn_interp_last_error": (C.c_char_p, [_P]),
    "rn_interp_set_mask": (C.c_int, [_P, _P]),
    "rn_interp_is_symmetric": (C.c_int, [_P]),
    "rn_interp_calc_polarizabilities": (C.c_int, [_P, _P, C.c_int64, _P]),
    "rn_interp_forward_device": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "rn_interp_jacobian_device": (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    "rn_interp_group_increments_device": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int, C.c_size_t, _P, _P]),
    "rn_interp_mode_increments_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int32, C.c_int, C.c_size_t, _P, _P]),
    "rn_interp_partial_raman_tensors": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int, _P]),
}

# include/rn_lineshape.h (the Lorentzian fits of ramannoodle_amd/lineshape.py; a table of its own, as INTERP_SIGNATURES is)
LINESHAPE_SIGNATURES = {
    "rn_lineshape_fit": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, _P, _P, _P]),
    "rn_lineshape_fit_device": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, _P, _P, _P,
                                          _P]),
    "rn_lineshape_window_capacity": (C.c_int, []),
    "rn_lineshape_last_error": (C.c_char_p, []),
}

# include/rn_peakfit.h (the multi-peak fits of ramannoodle_amd/peakfit.py; a table of its own as well): the arguments of the
# two lineshape entries with (shape, linear, P, origin, centres, widths) after F
PEAKFIT_SIGNATURES = {
    "rn_peakfit_fit": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P,
                                 _P, _P, C.c_int, _P, _P, _P]),
    "rn_peakfit_fit_device": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, C.c_int,
                                        C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "rn_peakfit_window_capacity": (C.c_int, []),
    "rn_peakfit_last_error": (C.c_char_p, []),
}

# include/rn_quasiharmonic.h (the covariance moments of ramannoodle_amd/quasiharmonic.py; a table of its own as well)
QH_SIGNATURES = {
    "rn_qh_moments": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, _P]),
    "rn_qh_moments_device": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "rn_qh_chunk_frames": (C.c_int, []),
    "rn_qh_set_profiling": (C.c_int, [C.c_int]),
    "rn_qh_phase_times": (C.c_int, [_P]),
    "rn_qh_last_error": (C.c_char_p, []),
}

# include/rn_harmonic.h (the harmonic trajectories of ramannoodle_amd/harmonic.py; a table of its own as well)
HT_SIGNATURES = {
    "rn_ht_synthesize": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _P]),
    "rn_ht_synthesize_device": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                          C.c_int64, _P, _P]),
    "rn_ht_set_profiling": (C.c_int, [C.c_int]),
    "rn_ht_phase_times": (C.c_int, [_P]),
    "rn_ht_last_error": (C.c_char_p, []),
}

# include/rn_bandmodes.h (the band moments of ramannoodle_amd/bandmodes.py; a table of its own as well)
BM_SIGNATURES = {
    "rn_bm_moments": (C.c_int, [C.c_int, _P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64,
                                C.c_int64, C.c_size_t, _P]),
    "rn_bm_moments_device": (C.c_int, [C.c_int, _P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, C.c_int64, _P, _P,
                                       C.c_int64, C.c_int64, C.c_size_t, _P, _P]),
    "rn_bm_set_profiling": (C.c_int, [C.c_int]),
    "rn_bm_phase_times": (C.c_int, [_P]),
    "rn_bm_last_error": (C.c_char_p, []),
}

# include/rn_select.h (the nearest-reference distance and farthest-point selection of ramannoodle_amd/selection.py; a
# table of its own as well)
SELECT_SIGNATURES = {
    "rn_select_nearest": (C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P]),
    "rn_select_nearest_device": (C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, _P, C.c_int, _P, _P, _P]),
    "rn_select_farthest": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64, _P,
                                     _P]),
    "rn_select_farthest_device": (C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64,
                                            C.c_int64, _P, _P, _P]),
    "rn_select_tile_rows": (C.c_int, []),
    "rn_select_reference_splits": (C.c_int64, [C.c_int64, C.c_int64]),
    "rn_select_set_profiling": (C.c_int, [C.c_int]),
    "rn_select_phase_times": (C.c_int, [_P]),
    "rn_select_last_error": (C.c_char_p, []),
}

_lib = None


def library_path() -> str:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the shared library (once) and attach signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise DeviceError(
            f"{_LIB_PATH} not found: build it with ramannoodle_amd/csrc/build.sh "
            "(there is no CPU fallback for the PotGNN evaluation path)"
        )
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as exc:
        raise DeviceError(f"cannot load {_LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in (list(SIGNATURES.items()) + list(INTERP_SIGNATURES.items())
                                      + list(LINESHAPE_SIGNATURES.items()) + list(PEAKFIT_SIGNATURES.items())
                                      + list(QH_SIGNATURES.items())
                                      + list(HT_SIGNATURES.items()) + list(BM_SIGNATURES.items())
                                      + list(SELECT_SIGNATURES.items())):
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check_interp(rc: int, handle=None, what: str = "device call") -> None:
    """``check`` for the entries of ``include/rn_interp.h``, whose handles keep their own error text."""
    check(rc, handle, what, last_error="rn_interp_last_error")


def check_status(rc: int, what: str, last_error: str) -> None:
    """``check`` for the modules whose entries take no handle (the fits, the covariance moments, the harmonic
    trajectories, the band moments): ``last_error`` names the module's ``rn_*_last_error``, which takes no argument."""
    if rc == RN_OK:
        return
    text = (getattr(load(), last_error)() or b"").decode()
    if rc == RN_ERR_INVALID_ARGUMENT:
        raise ValueError(f"{what}: {text}")
    if rc == RN_ERR_OUT_OF_MEMORY:
        raise MemoryError(f"{what}: {text}")
    raise DeviceError(f"{what} failed ({rc}): {text}")


def check(rc: int, handle=None, what: str = "device call", last_error: str = "rn_potgnn_last_error") -> None:
    """Map a status code to the exception the reference API contract expects."""
    if rc == RN_OK:
        return
    lib = load()
    msg = getattr(lib, last_error)(handle)
    text = msg.decode() if msg else ""
    if rc == RN_ERR_INVALID_ARGUMENT:
        raise ValueError(f"{what}: {text}")
    if rc == RN_ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {text}")
    if rc == RN_ERR_OUT_OF_MEMORY:
        raise MemoryError(f"{what}: {text}")
    raise DeviceError(f"{what} failed ({rc}): {text}")
