"""The table of the guard-band tests (tests/test_guard_bands.py checks it against ``ramannoodle_amd/_lib.py``,
tests/test_guard_bands_gpu.py runs it): every C entry whose name ends in ``_device`` or ``_to_device``, how each of its
pointers is classified by the entry's header comment, how the first kernel behind it reads the caller's device pointers,
and the test of tests/test_guard_bands_gpu.py that hands it views inside guarded buffers.

``device``: the pointer arguments that are device memory (banded tensors in the test); ``host_out``: host results the
entry fills through a pointer (banded numpy arrays); every other pointer is a host input.  ``access``: what reading the
kernel found for an address that is aligned to its element only (8 bytes for float64, 4 for float32 and int32).  No
entry makes an access wider than an element on a caller's pointer: the ``float4`` / ``double2`` / LDS-DMA accesses of
the library are all on its own workspaces (node and edge rows, packed weights, FFT signals, LDS tiles), so no entry
has to refuse an element-aligned pointer.

``bitwise``: whether the entry documents bit-identical repeats.  Where it does not (the reverse pass of the evaluator
accumulates cotangents with atomics: ``include/rn_potgnn.h`` at ``rn_potgnn_group_increments_device``), the banded result
is compared with the plain one at the bar the entry's own repeat test uses, which ``repeat_bar`` names."""
from collections import namedtuple

Entry = namedtuple("Entry", "device host_out access test bitwise repeat_bar", defaults=(True, None))

_GEOMETRY = ("geom_rbf_kernel / geom_rbf_pairs_kernel (csrc/kernels_agg.hip) read positions, lattices and atom types one "
             "element at a time (pa[k], lat[k], types[row])")
_READOUT = "the readout kernels store alpha[s * 9 + c] and vec6[s * 6 + c] one element per thread"
_SIGNALS = ("the first kernel reads the series one element at a time into the FFT workspace; its double2 stores are on "
            "that workspace (hipfftDoubleComplex)")
_REVERSE = ("cast_from_f64_kernel reads the cotangents element by element; geom_input_bwd_kernel (csrc/kernels_bwd.hip) "
            "stores dpos / dlat one double at a time")

ENTRIES = {
    # ------------------------------------------------------------------ the evaluator (include/rn_potgnn.h)
    "rn_potgnn_forward_device": Entry(
        ("d_positions", "d_alpha", "d_vec6"), (), f"element-wide: {_GEOMETRY}; {_READOUT}", "test_potgnn_evaluation"),
    "rn_potgnn_forward_device_f64": Entry(
        ("d_positions", "d_alpha"), (), f"element-wide: {_GEOMETRY}; {_READOUT}", "test_potgnn_evaluation"),
    "rn_potgnn_forward_cells_device": Entry(
        ("d_positions", "d_lattices", "d_alpha"), (),
        f"element-wide: cast_from_f64_kernel reads the lattices element by element (float32 runs); {_GEOMETRY}; {_READOUT}",
        "test_potgnn_evaluation"),
    "rn_potgnn_calc_polarizabilities_to_device": Entry(
        ("d_alpha",), (), f"element-wide: {_READOUT}; the positions are host memory, staged by the entry",
        "test_potgnn_evaluation_to_device"),
    "rn_potgnn_calc_polarizabilities_cells_to_device": Entry(
        ("d_alpha",), (), f"element-wide: {_READOUT}; positions and lattices are host memory, staged by the entry",
        "test_potgnn_evaluation_to_device"),
    "rn_potgnn_forward_samples_device": Entry(
        ("d_lattices", "d_atom_types", "d_positions", "d_vec6"), (), f"element-wide: {_GEOMETRY}; node_init_kernel reads "
        f"types[row]; {_READOUT}", "test_potgnn_forward_samples"),
    "rn_potgnn_forward_vjp_device": Entry(
        ("d_lattices", "d_atom_types", "d_positions", "d_dvec6", "d_dpos", "d_dlat"), (),
        f"element-wide: {_GEOMETRY}; {_REVERSE}", "test_potgnn_forward_vjp", False,
        "tests/test_input_gradients.py::test_chunking_and_repeated_backward (1e-13 in float64) and "
        "::test_cuda_inputs_stay_on_device_and_respect_the_stream (1e-5 in float32)"),
    "rn_potgnn_group_increments_device": Entry(
        ("d_positions", "d_out"), (), f"element-wide: {_GEOMETRY}; group_increment_kernel (csrc/kernels_group.hip) reads "
        "x[t][i][r] and stores out[t][g][c] one double at a time", "test_potgnn_increments", False,
        "tests/test_chunk_walk_gpu.py::TOLERANCE"),
    "rn_potgnn_group_increments_cells_device": Entry(
        ("d_positions", "d_lattices", "d_out"), (), f"element-wide: as rn_potgnn_group_increments_device; cell_increment_kernel "
        "reads L[t][i][k] one double at a time", "test_potgnn_increments", False, "tests/test_chunk_walk_gpu.py::TOLERANCE"),
    "rn_potgnn_mode_increments_device": Entry(
        ("d_positions", "d_lattices", "d_out"), (), f"element-wide: {_GEOMETRY}; mode_increment_kernel (csrc/kernels_mode.hip) "
        "loads its tiles one double at a time from clamped addresses", "test_potgnn_increments", False,
        "tests/test_chunk_walk_gpu.py::TOLERANCE"),
    "rn_potgnn_mode_contract_device": Entry(
        ("d_jac", "d_positions", "d_disp", "d_proj", "d_out"), (), "element-wide: mode_increment_kernel "
        "(csrc/kernels_mode.hip) loads J, x, D and P one double at a time from clamped addresses and stores out[t][m][c] "
        "under t < steps && mode < M; mode_rest_kernel reads and writes single doubles", "test_mode_contract"),
    "rn_potgnn_train_forward_samples_device": Entry(
        ("d_lattices", "d_atom_types", "d_positions", "d_vec6"), (), f"element-wide: {_GEOMETRY}; the result reaches d_vec6 "
        "through a device-to-device copy of S * 6 floats", "test_potgnn_device_training"),
    "rn_potgnn_train_backward_samples_device": Entry(
        ("d_dvec6",), (), "element-wide: readout_bwd_kernel reads dout6[c * 6 + k]", "test_potgnn_device_training", False,
        "tests/test_input_gradients.py::_same_as_plain_step (1e-5 of the largest gradient)"),
    "rn_potgnn_train_backward_inputs_device": Entry(
        ("d_dvec6", "d_dpos", "d_dlat"), (), f"element-wide: readout_bwd_kernel reads dout6[c * 6 + k]; {_REVERSE}",
        "test_potgnn_device_training", False,
        "tests/test_input_gradients.py::_same_as_plain_step (1e-5 of the largest gradient)"),
    # ------------------------------------------------------------------ the spectrum reducers (include/rn_potgnn.h, rn_md_*)
    "rn_md_raman_intensities_device": Entry(("d_alpha",), ("intensities",), f"element-wide: {_SIGNALS}", "test_md_raman"),
    "rn_md_raman_polarized_device": Entry(("d_alpha",), ("out",), f"element-wide: {_SIGNALS}", "test_md_raman"),
    "rn_md_raman_segments_device": Entry(("d_alpha",), ("out",), f"element-wide: {_SIGNALS}", "test_md_raman"),
    "rn_md_raman_segments_at_device": Entry(("d_alpha",), ("out",), f"element-wide: {_SIGNALS}", "test_md_raman_ensemble"),
    "rn_md_raman_segment_replicates_device": Entry(("d_alpha",), ("out",), f"element-wide: {_SIGNALS}",
                                                   "test_md_raman_replicates"),
    "rn_md_raman_partial_device": Entry(("d_increments",), ("out",), f"element-wide: {_SIGNALS}", "test_md_partial"),
    "rn_md_raman_partial_segments_device": Entry(("d_increments",), ("out",), f"element-wide: {_SIGNALS}",
                                                 "test_md_partial"),
    "rn_md_vdos_device": Entry(("d_positions", "d_lattices"), ("out",), f"element-wide: {_SIGNALS}", "test_md_vdos"),
    "rn_md_mode_vdos_device": Entry(("d_positions", "d_lattices"), ("out",), "element-wide: project_steps_kernel "
                                    "(csrc/spectrum_mode_vdos.hip) loads positions and lattices one double at a time; its "
                                    "double2 stores are on the FFT workspace", "test_md_mode_vdos"),
    "rn_md_raman_modes_device": Entry(("d_increments",), ("out",), f"element-wide: {_SIGNALS}", "test_md_modes"),
    "rn_md_raman_mode_matrix_device": Entry(("d_increments",), ("out",), f"element-wide: {_SIGNALS}; the double2 accesses of "
                                            "csrc/spectrum_mode_matrix.hip are on LDS tiles and the transformed workspace",
                                            "test_md_modes"),
    # ------------------------------------------------------------------ the interpolation model (include/rn_interp.h)
    "rn_interp_forward_device": Entry(("d_positions", "d_alpha"), (), "element-wide: interp_alpha_kernel "
                                      "(csrc/kernels_interp.hip) loads x[s][k] one double at a time from clamped addresses",
                                      "test_interp_forward_and_jacobian"),
    "rn_interp_jacobian_device": Entry(("d_positions", "d_jac"), (), "element-wide: as rn_interp_forward_device; "
                                       "interp_rows_kernel stores jac[row * 3N + col] one double at a time under row < R "
                                       "&& col < 3N",
                                       "test_interp_forward_and_jacobian"),
    "rn_interp_group_increments_device": Entry(("d_positions", "d_out"), (), "element-wide: as rn_interp_forward_device; "
                                               "group_increment_kernel (csrc/kernels_group.hip) is lane-strided over doubles",
                                               "test_interp_group_increments"),
    "rn_interp_mode_increments_device": Entry(("d_positions", "d_out"), (), "element-wide: as rn_interp_forward_device; "
                                              "mode_increment_kernel as for rn_potgnn_mode_contract_device",
                                              "test_interp_mode_increments"),
    # ------------------------------------------------------------------ the analysis entries
    "rn_lineshape_fit_device": Entry(("d_rows",), ("out", "status", "iterations"), "element-wide: lineshape_fit_kernel "
                                     "(csrc/lineshape.hip) reads rows[row * bins + first + i] one double per lane",
                                     "test_line_shape_fits"),
    "rn_peakfit_fit_device": Entry(("d_rows",), ("out", "status", "iterations"), "element-wide: peakfit_kernel "
                                   "(csrc/peakfit.hip) reads rows[row * bins + first + i] one double per lane",
                                   "test_line_shape_fits"),
    "rn_qh_moments_device": Entry(("d_positions",), ("first", "second", "counts"), "element-wide: covariance_chunk_kernel "
                                  "(csrc/kernels_covariance.hip) loads x[t][j] one double at a time from clamped addresses",
                                  "test_quasiharmonic_moments"),
    "rn_ht_synthesize_device": Entry(("d_out",), (), "element-wide: harmonic_synthesis_kernel (csrc/kernels_harmonic.hip) "
                                     "stores out[r][t][j] one double per lane under live && t < T", "test_harmonic_synthesis"),
    "rn_bm_moments_device": Entry(("d_positions", "d_alpha"), ("moments",), "element-wide: band_transform_kernel "
                                  "(csrc/kernels_band.hip) loads f[t][i][r] and alpha[t][c] one double at a time",
                                  "test_band_moments"),
}

# entries none of whose pointer arguments is device memory
EXEMPT = {
    "rn_potgnn_train_backward_device": "its only pointer, dvec6, is host memory (the gradients it leaves on the device are "
                                       "the library's own buffer)",
}


def device_entry_names():
    """Every name of the tables of ``ramannoodle_amd/_lib.py`` that ends in ``_device`` or ``_to_device``, and the
    float64 twin of such an entry (``_device_f64``)."""
    from ramannoodle_amd import _lib
    tables = (_lib.SIGNATURES, _lib.INTERP_SIGNATURES, _lib.LINESHAPE_SIGNATURES, _lib.PEAKFIT_SIGNATURES,
              _lib.QH_SIGNATURES, _lib.HT_SIGNATURES, _lib.BM_SIGNATURES)
    return sorted(name for table in tables for name in table if name.endswith(("_device", "_to_device", "_device_f64")))
