"""Raman spectra from Raman tensors (phonons) or a polarizability time series (MD).

Host-side numpy/scipy post-processing of the device results, kept on the CPU as the
scope table prescribes (ms-scale even at 10^4 frames).
Follows ``ramannoodle/spectrum/_raman.py`` and ``ramannoodle/spectrum/utils.py``.
"""
from __future__ import annotations

import numpy as np
import scipy.fftpack
import scipy.signal
from numpy.typing import NDArray

from ramannoodle_amd.abstract import RamanSpectrum
from ramannoodle_amd.constants import BOLTZMANN_CONSTANT
from ramannoodle_amd.exceptions import get_type_error, shape_string, verify_ndarray_shape

_CM1_TO_HZ = 29979245800.0
_PLANCK_EV_S = 4.1357e-15  # value used by the reference (spectrum/_raman.py:37)
_PER_FS_TO_CM1 = 33.35640951981521 * 1e3  # spectrum/utils.py:118-121


def get_bose_einstein_correction(wavenumbers: NDArray[np.float64],
                                 temperature: float) -> NDArray[np.float64]:
    """``1 / (1 - exp(-E/kT))`` (``spectrum/_raman.py:13-40``)."""
    try:
        if temperature <= 0:
            raise ValueError(f"invalid temperature: {temperature} <= 0")
    except TypeError as exc:
        raise get_type_error("temperature", temperature, "float") from exc
    try:
        energy = wavenumbers * _CM1_TO_HZ * _PLANCK_EV_S
        return 1 / (1 - np.exp(-energy / (BOLTZMANN_CONSTANT * temperature)))
    except TypeError as exc:
        raise get_type_error("wavenumbers", wavenumbers, "ndarray") from exc


def get_laser_correction(wavenumbers: NDArray[np.float64],
                         laser_wavenumber: float) -> NDArray[np.float64]:
    """``((nu - nu_L)/1e4)^4 / nu`` (``spectrum/_raman.py:43-69``)."""
    try:
        if laser_wavenumber <= 0:
            raise ValueError(f"invalid laser_wavenumber: {laser_wavenumber} <= 0")
    except TypeError as exc:
        raise get_type_error("laser_wavenumber", laser_wavenumber, "float") from exc
    try:
        return ((wavenumbers - laser_wavenumber) / 10000) ** 4 / wavenumbers
    except TypeError as exc:
        raise get_type_error("wavenumbers", wavenumbers, "ndarray") from exc


def _apply_corrections(wavenumbers, intensities, laser_correction, laser_wavelength,
                       bose_einstein_correction, temperature):
    if laser_correction:
        intensities = intensities * get_laser_correction(wavenumbers, 10000000 / laser_wavelength)
    if bose_einstein_correction:
        intensities = intensities * get_bose_einstein_correction(wavenumbers, temperature)
    return intensities


def _require_polycrystalline(orientation) -> None:
    if not (isinstance(orientation, str) and orientation == "polycrystalline"):
        raise NotImplementedError("only polycrystalline spectra are supported for now")


# ----------------------------------------------------------------------------- polarized spectra
# The six components of a symmetric tensor, in the order the device entry uses, and the 21 pairs
# (j <= l) of them, packed row-major over the upper triangle (include/rn_potgnn.h).
_COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))
_PAIRS = tuple((j, l) for j in range(6) for l in range(j, 6))
_PAIR_J = np.array([j for j, _ in _PAIRS])
_PAIR_L = np.array([l for _, l in _PAIRS])
_PAIR_SCALE = np.where(_PAIR_J == _PAIR_L, 1.0, 2.0)  # off-diagonal entries of M appear twice
# quadratic forms over the components: a^2 = ((xx+yy+zz)/3)^2 and the anisotropy gamma^2 of measure()
_ISO_FORM = np.zeros((6, 6))
_ISO_FORM[:3, :3] = 1.0 / 9.0
_ANISO_FORM = np.diag([1.0, 1.0, 1.0, 3.0, 3.0, 3.0])
_ANISO_FORM[:3, :3] -= 0.5 * (1.0 - np.eye(3))


def _symmetric_components(tensors: NDArray[np.float64]) -> NDArray[np.float64]:
    """``(..., 3, 3)`` -> ``(..., 6)``: (xx, yy, zz, xy, yz, xz) of the symmetric part."""
    return np.stack([0.5 * (tensors[..., a, b] + tensors[..., b, a]) for a, b in _COMPONENTS], axis=-1)


def _polarization_vectors(name: str, value) -> NDArray[np.float64]:
    if value is None or isinstance(value, (str, bytes)):
        raise get_type_error(name, value, "ndarray")
    try:
        array = np.asarray(value)
    except (TypeError, ValueError) as exc:
        raise get_type_error(name, value, "ndarray") from exc
    if array.dtype.kind not in "iuf":
        raise get_type_error(name, value, "ndarray of real numbers")
    array = array.astype(np.float64)
    if array.ndim not in (1, 2) or array.shape[-1] != 3:
        raise ValueError(f"{name} has wrong shape: {shape_string(array.shape)} != (3,) or (_,3)")
    if not np.all(np.isfinite(array)):
        raise ValueError(f"{name} is not finite")
    norms = np.linalg.norm(array, axis=-1)
    if np.any(norms == 0):
        raise ValueError(f"{name} holds a zero vector")
    return array / norms[..., None]


def _orientations(orientation):
    """``None`` -> identity, ``"polycrystalline"`` -> that string, else validated rotations."""
    if orientation is None:
        return np.eye(3)
    if isinstance(orientation, str):
        if orientation != "polycrystalline":
            raise ValueError(f"unknown orientation: {orientation!r}")
        return orientation
    try:
        array = np.asarray(orientation)
    except (TypeError, ValueError) as exc:
        raise get_type_error("orientation", orientation, "ndarray or str") from exc
    if array.dtype.kind not in "iuf":
        raise get_type_error("orientation", orientation, "ndarray or str")
    array = array.astype(np.float64)
    if array.ndim not in (2, 3) or array.shape[-2:] != (3, 3):
        raise ValueError(f"orientation has wrong shape: {shape_string(array.shape)} != (3,3) or (_,3,3)")
    if not np.all(np.isfinite(array)):
        raise ValueError("orientation is not finite")
    deviation = np.linalg.norm(array @ np.swapaxes(array, -1, -2) - np.eye(3), axis=(-2, -1))
    if np.any(deviation > 1e-8) or np.any(np.linalg.det(array) < 0):
        raise ValueError("orientation is not a proper rotation")
    return array


def polarized_weights(incident, scattered, orientation=None) -> tuple[NDArray[np.float64], bool]:
    """The packed weights ``W[K][21]`` of ``measure_polarized`` and whether the result is squeezed.

    Configuration k's intensity is ``sum_p W[k,p] C_p`` over the 21 component pairs ``p = (j,l)``,
    ``j <= l``, of (xx, yy, zz, xy, yz, xz) (``include/rn_potgnn.h``), where ``C_p`` is the spectrum of
    the symmetrised cross-correlation of components j and l (phonons: the product ``T_j T_l``); ``W`` packs
    a symmetric 6x6 form ``M`` with its off-diagonal entries doubled.  For one orientation R, ``M = w w^T``
    with ``w = (v0 u0, v1 u1, v2 u2, v0 u1 + v1 u0, v1 u2 + v2 u1, v0 u2 + v2 u0)``, ``u = R^T e_i``,
    ``v = R^T e_s``; for ``"polycrystalline"`` it is the isotropic average
    ``c^2 a^2 + (3 + c^2) gamma^2 / 45``, ``c = e_i . e_s``.  Every class builds its weights here.
    """
    e_i = _polarization_vectors("incident", incident)
    e_s = _polarization_vectors("scattered", scattered)
    rotations = _orientations(orientation)
    counts = [a.shape[0] for a in (e_i, e_s) if a.ndim == 2]
    if not isinstance(rotations, str) and rotations.ndim == 3:
        counts.append(rotations.shape[0])
    if len(set(counts)) > 1:
        raise ValueError(f"incident, scattered and orientation disagree on the number of configurations: {counts}")
    k = counts[0] if counts else 1
    e_i = np.broadcast_to(e_i, (k, 3))
    e_s = np.broadcast_to(e_s, (k, 3))
    if isinstance(rotations, str):
        c2 = np.einsum("ka,ka->k", e_i, e_s) ** 2
        forms = c2[:, None, None] * _ISO_FORM + ((3.0 + c2) / 45.0)[:, None, None] * _ANISO_FORM
        weights = forms[:, _PAIR_J, _PAIR_L] * _PAIR_SCALE
    else:
        rotations = np.broadcast_to(rotations, (k, 3, 3))
        u = np.einsum("kab,ka->kb", rotations, e_i)  # R^T e_i: crystal-frame components
        v = np.einsum("kab,ka->kb", rotations, e_s)
        outer = v[:, :, None] * u[:, None, :]
        w = _symmetric_components(outer) * np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
        weights = w[:, _PAIR_J] * w[:, _PAIR_L] * _PAIR_SCALE
    return np.ascontiguousarray(weights, dtype=np.float64), not counts


def _md_basis_spectra(polarizability_ts: NDArray[np.float64], timestep: float):
    """(wavenumbers, ``C[21][bins]``) on the host: calc_signal_spectrum's transform of the symmetrised
    cross-correlation of each component pair of the symmetric part of d(alpha)/dt, zero bin dropped."""
    d = _symmetric_components(np.diff(polarizability_ts, axis=0))
    n = d.shape[0]
    wavenumbers = scipy.fftpack.fftfreq(n, timestep) * _PER_FS_TO_CM1
    keep = np.flatnonzero(wavenumbers >= 0)[1:]
    basis = np.empty((len(_PAIRS), len(keep)))
    for p, (j, l) in enumerate(_PAIRS):
        full = scipy.signal.correlate(d[:, j], d[:, l], "full")
        lags = 0.5 * (full[n - 1:] + full[n - 1::-1])
        basis[p] = np.real(scipy.fftpack.fft(lags))[keep]
    return wavenumbers[keep], basis


def _lag_axis(n: int, timestep: float):
    """What the host reducers of ``n`` differences per segment start from: ``(wavenumbers, keep, length)``, the kept
    wavenumbers (the positive ones of a length-``n`` transform), their bins and the padded transform length."""
    wavenumbers = scipy.fftpack.fftfreq(n, timestep) * _PER_FS_TO_CM1
    keep = np.flatnonzero(wavenumbers >= 0)[1:]
    return wavenumbers[keep], keep, 1 << int(np.ceil(np.log2(max(2 * n - 1, 1))))


def _lag_spectrum(power, n: int, length: int, keep):
    """The back half of the host reducers: power spectra on the padded length ``(..., length / 2 + 1)`` -> the positive
    lags of the autocorrelation, their length-``n`` transform, the real bins ``keep``: ``(..., bins)``."""
    lags = np.fft.irfft(power, n=length, axis=-1)[..., :n]
    return np.real(scipy.fftpack.fft(lags, axis=-1))[..., keep]


def _call_md_reducer(entry: str, source, n: int, too_short: str, timestep: float, device: int, stream,
                     out_shape, args_before=(), args_after=(), bin_axis: bool = True):
    """What every device reduction shares.  ``source`` is a host array (entry ``entry``) or, with ``stream`` set, a
    contiguous float64 CUDA tensor (entry ``entry + "_device"``, ordered after ``stream``); ``n`` is the number of
    differences of the series.  The call is ``entry(source, *args_before, device, *args_after, out, bins[, stream])``
    with ``out`` a new float64 array ``(*out_shape, bins)``, or ``out_shape`` itself with ``bin_axis=False``.  Returns
    ``(wavenumbers, out)``."""
    import ctypes as C

    from ramannoodle_amd import _lib
    if n < 2:
        raise ValueError(too_short)
    bins = (n + 1) // 2 - 1
    out = np.empty((*out_shape, bins) if bin_axis else tuple(out_shape), dtype=np.float64)
    if stream is None:
        source = np.ascontiguousarray(source, dtype=np.float64)
        pointer, tail = source.ctypes.data, ()
    else:
        entry += "_device"
        pointer, tail = source.data_ptr(), (C.c_void_p(stream),)
    rc = getattr(_lib.load(), entry)(C.c_void_p(pointer), *args_before, device, *args_after,
                                     C.c_void_p(out.ctypes.data), bins, *tail)
    _lib.check(rc, None, entry)
    wavenumbers = scipy.fftpack.fftfreq(n, timestep) * _PER_FS_TO_CM1
    return wavenumbers[1:bins + 1], out


def _weights_arguments(weights):
    """``(contiguous float64 weights, their (pointer, K) arguments)``."""
    import ctypes as C
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    return weights, (C.c_void_p(weights.ctypes.data), weights.shape[0])


_TOO_FEW_STEPS = "the device reduction needs at least three time steps"


def _md_polarized_on_device(alpha, timestep: float, weights, device: int, stream=None,
                            workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K][bins]``) from ``rn_md_raman_polarized`` (host alpha) or, with a
    torch CUDA tensor, ``rn_md_raman_polarized_device`` ordered after ``stream``."""
    weights, weight_args = _weights_arguments(weights)
    return _call_md_reducer("rn_md_raman_polarized", alpha, alpha.shape[0] - 1, _TOO_FEW_STEPS, timestep, device,
                            stream, (weights.shape[0],), (alpha.shape[0], *weight_args), (workspace_limit,))


def calc_signal_spectrum(signal: NDArray[np.float64],
                         sampling_rate: float) -> tuple[NDArray[np.float64], NDArray[np.float64]]:
    """Non-negative-frequency FFT of the positive-lag autocorrelation
    (``spectrum/utils.py:76-124``)."""
    verify_ndarray_shape("signal", signal, (None,))
    full = scipy.signal.correlate(signal, signal, "full")
    autocorrelation = full[(len(full) - 1) // 2:]
    wavenumbers = scipy.fftpack.fftfreq(autocorrelation.size, sampling_rate) * _PER_FS_TO_CM1
    intensities = np.real(scipy.fftpack.fft(autocorrelation))
    keep = wavenumbers >= 0
    return wavenumbers[keep], intensities[keep]


def convolve_spectrum(wavenumbers, intensities, function: str = "gaussian", width: float = 5,
                      out_wavenumbers=None):
    """Gaussian / Lorentzian broadening (``spectrum/utils.py:13-73``)."""
    if out_wavenumbers is None:
        lo, hi = np.min(wavenumbers) - 100, np.max(wavenumbers) + 100
        out_wavenumbers = np.linspace(lo, hi, int(np.rint(hi - lo)))
    verify_ndarray_shape("out_wavenumbers", out_wavenumbers, (None,))
    verify_ndarray_shape("wavenumbers", wavenumbers, (None,))
    verify_ndarray_shape("intensities", intensities, (len(wavenumbers),))
    try:
        if width <= 0:
            raise ValueError(f"invalid width: {width} <= 0")
    except TypeError as exc:
        raise get_type_error("width", width, "float") from exc
    if function not in ("gaussian", "lorentzian"):
        raise ValueError(f"unsupported convolution type: {function}")
    delta = np.asarray(wavenumbers)[:, None] - out_wavenumbers[None, :]
    if function == "gaussian":
        kernel = (1 / width) * (1 / np.sqrt(2 * np.pi)) * np.exp(-(delta**2) / (2 * width**2))
    else:
        kernel = (1 / np.pi) * (0.5 * width / (delta**2 + (0.5 * width) ** 2))
    return out_wavenumbers, (kernel * np.asarray(intensities)[:, None]).sum(axis=0)


def _md_intensities_on_device(polarizability_ts, timestep: float, device: int, stream=None):
    """(wavenumbers, uncorrected intensities) of ``MDRamanSpectrum.measure`` from ``rn_md_raman_intensities`` (a host
    series) or, with a torch CUDA tensor ``float64[S,3,3]``, ``rn_md_raman_intensities_device`` ordered after ``stream``:
    then only the intensities reach the host."""
    steps = polarizability_ts.shape[0]
    return _call_md_reducer("rn_md_raman_intensities", polarizability_ts, steps - 1, _TOO_FEW_STEPS, timestep, device,
                            stream, (), (steps,))


# ----------------------------------------------------------------------------- segment (Welch / time-resolved) spectra
_TAPERS = ("boxcar", "hann", "hamming", "blackman")


def segment_plan(steps: int, segment_steps, hop=None, taper="hann") -> tuple[int, int, NDArray[np.float64]]:
    """Resolve the segmentation of a series of ``steps`` polarizabilities into ``(W, H, tau)``.

    ``segment_steps = W`` polarizabilities per segment (an int, ``3 <= W <= steps``), ``hop = H >= 1`` steps between
    segment starts (default ``W // 2``), ``taper``: ``"boxcar"``, ``"hann"``, ``"hamming"``, ``"blackman"`` (the symmetric
    forms, ``scipy.signal.get_window(name, W - 1, fftbins=False)``) or a real array ``(W - 1,)``.  ``tau`` is the taper
    over the ``W - 1`` differences of a segment, normalised to ``mean(tau^2) = 1`` (a taper whose mean square is zero,
    such as ``"hann"`` at ``W = 3``, is a ``ValueError``).  Every segment spectrum path resolves its arguments here."""
    if isinstance(segment_steps, (bool, np.bool_)) or not isinstance(segment_steps, (int, np.integer)):
        raise get_type_error("segment_steps", segment_steps, "int")
    width = int(segment_steps)
    if width < 3:
        raise ValueError(f"invalid segment_steps: {width} < 3")
    if width > steps:
        raise ValueError(f"invalid segment_steps: {width} > {steps} time steps")
    if hop is None:
        hop = width // 2
    if isinstance(hop, (bool, np.bool_)) or not isinstance(hop, (int, np.integer)):
        raise get_type_error("hop", hop, "int")
    hop = int(hop)
    if hop < 1:
        raise ValueError(f"invalid hop: {hop} < 1")
    n = width - 1
    if isinstance(taper, str):
        if taper not in _TAPERS:
            raise ValueError(f"unknown taper: {taper!r} (one of {', '.join(_TAPERS)}, or an array ({n},))")
        tau = scipy.signal.get_window(taper, n, fftbins=False).astype(np.float64)
    else:
        if taper is None or isinstance(taper, bytes):
            raise get_type_error("taper", taper, "str or ndarray")
        try:
            tau = np.asarray(taper)
        except (TypeError, ValueError) as exc:
            raise get_type_error("taper", taper, "str or ndarray") from exc
        if tau.dtype.kind not in "iuf":
            raise get_type_error("taper", taper, "str or ndarray of real numbers")
        if tau.shape != (n,):
            raise ValueError(f"taper has wrong shape: {shape_string(tau.shape)} != ({n},)")
        tau = tau.astype(np.float64)
        if not np.all(np.isfinite(tau)):
            raise ValueError("taper is not finite")
    mean_square = float(np.mean(tau * tau))
    if not mean_square > 0.0:
        raise ValueError(f"taper has mean(taper^2) == 0 over the {n} differences of a segment")
    return width, hop, np.ascontiguousarray(tau / np.sqrt(mean_square))


def _segment_starts(steps: int, width: int, hop: int) -> NDArray[np.int64]:
    return np.arange((steps - width) // hop + 1, dtype=np.int64) * hop


_SEGMENT_CHUNK_ELEMENTS = 1 << 23  # complex spectra held at once by the host path


def _md_segments_host(polarizability_ts, timestep: float, weights, width: int, hop, tau, average: bool, starts=None):
    """(wavenumbers, ``I[K][bins]`` or ``I[Q][K][bins]``) on the host, from the definition (``include/rn_potgnn.h``,
    ``rn_md_raman_segments``): per segment the zero-padded transforms of the six tapered difference components, the
    contracted power spectrum of each configuration, its inverse transform, the positive lags and their length-n
    transform; the mean over the segments is taken on the power spectra.  ``starts`` (the first step of each segment,
    ``rn_md_raman_segments_at``) replaces the grid of ``hop``: a table that respects the run boundaries of a
    concatenated series never reads a difference across one."""
    d = _symmetric_components(np.diff(np.asarray(polarizability_ts, dtype=np.float64), axis=0))  # (S - 1, 6)
    n = width - 1
    if starts is None:
        starts = _segment_starts(d.shape[0] + 1, width, hop)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    count = weights.shape[0]

    rows = None if average else np.empty((len(starts), count, len(keep)))
    mean = np.zeros((count, length // 2 + 1))
    chunk = max(1, _SEGMENT_CHUNK_ELEMENTS // ((length // 2 + 1) * max(count, len(_PAIRS))))
    for first in range(0, len(starts), chunk):
        index = starts[first:first + chunk, None] + np.arange(n)[None, :]
        spectra = np.fft.rfft(d[index] * tau[None, :, None], n=length, axis=1)  # (q, length / 2 + 1, 6)
        cross = np.real(spectra[:, :, _PAIR_J] * np.conj(spectra[:, :, _PAIR_L]))
        power = np.einsum("kp,qfp->qkf", weights, cross)
        if average:
            mean += power.sum(axis=0)
        else:
            rows[first:first + chunk] = _lag_spectrum(power, n, length, keep)
    return wavenumbers, _lag_spectrum(mean / len(starts), n, length, keep) if average else rows


def _md_segments_on_device(alpha, timestep: float, weights, width: int, hop: int, tau, average: bool, device: int,
                           stream=None, workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K][bins]`` or ``I[Q][K][bins]``) from ``rn_md_raman_segments`` (host alpha) or, with
    a torch CUDA tensor, ``rn_md_raman_segments_device`` ordered after ``stream``."""
    import ctypes as C
    steps = alpha.shape[0]
    weights, weight_args = _weights_arguments(weights)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    shape = (weights.shape[0],) if average else ((steps - width) // hop + 1, weights.shape[0])
    return _call_md_reducer("rn_md_raman_segments", alpha, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
                            (steps, width, hop, C.c_void_p(tau.ctypes.data), *weight_args, int(bool(average))),
                            (workspace_limit,))


def ensemble_segment_starts(run_lengths, segment_steps, hop=None) -> tuple[NDArray[np.int64], NDArray[np.int64]]:
    """The segments of several runs joined end to end: ``(starts, run_index)``, both ``int64[Q]``.

    ``run_lengths``: the number of steps ``S_r`` of each run; ``segment_steps`` and ``hop`` as in ``segment_plan``.
    Run r contributes its own ``(S_r - segment_steps) // hop + 1`` segments, in run order; ``starts`` counts steps of
    the concatenated series (the run's offset plus the start within the run) and ``run_index`` names the run, so no
    segment crosses a run boundary.  A run shorter than ``segment_steps`` is a ``ValueError``."""
    lengths = [int(length) for length in run_lengths]
    if not lengths:
        raise ValueError("an ensemble needs at least one run")
    starts, run_index, offset = [], [], 0
    for run, length in enumerate(lengths):
        width, step, _ = segment_plan(length, segment_steps, hop, "boxcar")
        own = _segment_starts(length, width, step)
        starts.append(own + offset)
        run_index.append(np.full(len(own), run, dtype=np.int64))
        offset += length
    return np.concatenate(starts), np.concatenate(run_index)


def _table_arguments(starts):
    """``(contiguous int64 starts, their (pointer, Q) arguments)``."""
    import ctypes as C
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    return starts, (C.c_void_p(starts.ctypes.data), starts.shape[0])


def _md_segments_at_on_device(alpha, timestep: float, weights, width: int, starts, tau, average: bool, device: int,
                              stream=None, workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K][bins]`` or ``I[Q][K][bins]``) from ``rn_md_raman_segments_at`` (host alpha) or,
    with a torch CUDA tensor, ``rn_md_raman_segments_at_device`` ordered after ``stream``."""
    import ctypes as C
    weights, weight_args = _weights_arguments(weights)
    starts, table_args = _table_arguments(starts)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    shape = (weights.shape[0],) if average else (len(starts), weights.shape[0])
    return _call_md_reducer("rn_md_raman_segments_at", alpha, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
                            (alpha.shape[0], width, *table_args, C.c_void_p(tau.ctypes.data), *weight_args,
                             int(bool(average))), (workspace_limit,))


class PhononRamanSpectrum(RamanSpectrum):
    """First-order spectrum from phonon wavenumbers ``(M,)`` and Raman tensors ``(M,3,3)``
    (``spectrum/_raman.py:72-194``)."""

    def __init__(self, phonon_wavenumbers, raman_tensors) -> None:
        verify_ndarray_shape("phonon_wavenumbers", phonon_wavenumbers, (None,))
        verify_ndarray_shape("raman_tensors", raman_tensors, (len(phonon_wavenumbers), 3, 3))
        self._phonon_wavenumbers = phonon_wavenumbers
        self._raman_tensors = raman_tensors

    @property
    def phonon_wavenumbers(self):
        return self._phonon_wavenumbers.copy()

    @property
    def raman_tensors(self):
        return self._raman_tensors.copy()

    def measure(self, orientation="polycrystalline", laser_correction=False,
                laser_wavelength=522, bose_einstein_correction=False, temperature=300):
        _require_polycrystalline(orientation)
        r = self._raman_tensors
        xx, yy, zz = r[:, 0, 0], r[:, 1, 1], r[:, 2, 2]
        alpha_squared = ((xx + yy + zz) / 3.0) ** 2
        gamma_squared = (
            (xx - yy) ** 2 + (xx - zz) ** 2 + (yy - zz) ** 2
            + 6.0 * (r[:, 0, 1] ** 2 + r[:, 0, 2] ** 2 + r[:, 1, 2] ** 2)
        ) / 2.0
        intensities = 45.0 * alpha_squared + 7.0 * gamma_squared
        intensities = _apply_corrections(self._phonon_wavenumbers, intensities, laser_correction,
                                         laser_wavelength, bose_einstein_correction, temperature)
        return self._phonon_wavenumbers, intensities

    def measure_polarized(self, incident, scattered, orientation=None, laser_correction=False,
                          laser_wavelength=522, bose_einstein_correction=False, temperature=300, device=None):
        """Intensities ``(e_s . R T_m R^T . e_i)^2`` of each mode for set polarizations (an addition).

        ``incident`` / ``scattered``: lab-frame vectors ``(3,)`` or ``(K,3)``, normalised here (a zero
        vector is a ``ValueError``); ``orientation``: ``None`` (identity), a proper rotation ``(3,3)`` or
        ``(K,3,3)`` taking crystal-frame components to the lab frame, or ``"polycrystalline"`` (the
        isotropic average, ``c^2 a^2 + (3 + c^2) gamma^2 / 45`` with ``c = e_i . e_s``; so
        ``45 (I_parallel + I_perpendicular)`` is ``measure()``).  ``K`` broadcasts across the three.
        The symmetric part of each Raman tensor is used.  Returns ``(wavenumbers, intensities)`` with
        intensities ``(K, M)``, or ``(M,)`` when no argument has a ``K`` axis; the corrections apply to
        each row as in ``measure``.  ``device`` is accepted for a signature common to all spectra; the
        reduction of at most 3N modes always runs on the host.
        """
        del device
        weights, squeeze = polarized_weights(incident, scattered, orientation)
        d = _symmetric_components(np.asarray(self._raman_tensors, dtype=np.float64))
        intensities = weights @ (d[:, _PAIR_J] * d[:, _PAIR_L]).T
        intensities = _apply_corrections(self._phonon_wavenumbers, intensities, laser_correction,
                                         laser_wavelength, bose_einstein_correction, temperature)
        return self._phonon_wavenumbers, intensities[0] if squeeze else intensities


# ----------------------------------------------------------------------------- the time series of an MD spectrum
def _run_offsets(run_lengths) -> NDArray[np.int64]:
    return np.concatenate([[0], np.cumsum(run_lengths)[:-1]]).astype(np.int64)


def _equal_run_length(run_lengths) -> int:
    if len(set(run_lengths)) != 1:
        raise ValueError(f"the mean of the runs' whole spectra needs runs of one length, not {sorted(set(run_lengths))}: "
                         "use measure_segments")
    return run_lengths[0]


class _Series:
    """The time series of an MD spectrum class, and the only thing that knows where it lives.

    ``data`` is a host ndarray or a contiguous float64 CUDA tensor, time along the first axis.  Its rows are frames, or
    with ``increments`` the differences between successive frames (frame t is where increment t begins).
    ``run_lengths`` is ``None`` for a single run, or the frames of each of several runs joined end to end; runs of
    increments are joined with one row between them (zeros, or whatever a batched evaluation of the joined frames wrote
    there), so that increment t still belongs to frame t of the joined frames, and no segment reads that row."""

    def __init__(self, data, run_lengths=None, increments: bool = False):
        self.data = data
        self.run_lengths = run_lengths
        self.increments = increments
        self._host_copy = None
        self._whole_table = None

    @classmethod
    def of_tensor(cls, name: str, tensor, pattern, run_lengths=None, increments: bool = False):
        """A CUDA tensor shaped like ``pattern`` (``None``: any size), contiguous and float64."""
        shape = tuple(tensor.shape)
        if len(shape) != len(pattern) or any(want is not None and have != want for have, want in zip(shape, pattern)):
            raise ValueError(f"{name} has wrong shape: {shape} != {shape_string(pattern)}")
        if not (tensor.is_cuda and tensor.is_contiguous() and str(tensor.dtype) == "torch.float64"):
            raise ValueError(f"{name} must be a contiguous float64 CUDA tensor")
        return cls(tensor, run_lengths, increments)

    @classmethod
    def of_runs(cls, runs, trailing, shared_axis: bool, increments: bool = False):
        """Host runs joined end to end as float64: each ``(S_r, *trailing)``, or with ``shared_axis``
        ``(S_r, A, *trailing)`` for the first run's ``A``."""
        runs = list(runs)
        if not runs:
            raise ValueError("an ensemble needs at least one run")
        pattern = (None, runs[0].shape[1], *trailing) if shared_axis else (None, *trailing)
        for index, run in enumerate(runs):
            verify_ndarray_shape(f"runs[{index}]", run, pattern)
        parts = [np.asarray(run, dtype=np.float64) for run in runs]
        if increments:
            gap = np.zeros((1, *runs[0].shape[1:]))
            parts = [part for run in parts for part in (run, gap)][:-1]
        lengths = [int(run.shape[0]) + int(increments) for run in runs]
        return cls(np.concatenate(parts, axis=0), lengths, increments)

    @classmethod
    def of_tensor_runs(cls, name: str, runs, run_lengths, pattern, increments: bool = False, tensors_only: bool = False):
        """Device runs: a sequence of CUDA tensors, joined here on the GPU, or one tensor holding them end to end with
        ``run_lengths`` (frames per run; joined increments have ``sum(run_lengths) - 1`` rows)."""
        import torch
        if isinstance(runs, torch.Tensor):
            if run_lengths is None:
                raise ValueError("runs: one joined tensor needs run_lengths")
            lengths = [int(length) for length in run_lengths]
            if not lengths or min(lengths) < 1 or sum(lengths) - int(increments) != runs.shape[0]:
                raise ValueError(f"runs: run_lengths {lengths} do not add up to the {runs.shape[0]} rows of the tensor")
            return cls.of_tensor(name, runs, pattern, lengths, increments)
        if run_lengths is not None:
            raise ValueError("runs: run_lengths goes with one joined tensor, not with a sequence of runs")
        runs = list(runs)
        if not runs:
            raise ValueError("an ensemble needs at least one run")
        if tensors_only and not all(isinstance(run, torch.Tensor) for run in runs):
            raise ValueError("runs must be contiguous float64 CUDA tensors")
        lengths = [int(run.shape[0]) + int(increments) for run in runs]
        if increments:
            gap = runs[0].new_zeros((1, *runs[0].shape[1:]))
            joined = torch.cat([part for run in runs for part in (run, gap)][:-1], dim=0)
        else:
            joined = runs[0] if len(runs) == 1 else torch.cat(runs, dim=0)
        return cls.of_tensor(name, joined, pattern, lengths, increments)

    # -------------------------------------------------------------------------------------------------- access
    @property
    def shape(self) -> tuple:
        return tuple(self.data.shape)

    @property
    def frames(self) -> int:
        """Frames of the series, run boundaries included."""
        return int(self.data.shape[0]) + int(self.increments)

    @property
    def gpu(self):
        """The index of the GPU that holds the series, ``None`` for a host array."""
        if not getattr(self.data, "is_cuda", False):
            return None
        return self.data.device.index or 0

    def host(self):
        """The series as a host array: a tensor is copied on first use."""
        if self.gpu is None:
            return self.data
        if self._host_copy is None:
            self._host_copy = self.data.cpu().numpy()
        return self._host_copy

    def source(self, device: int):
        """``(source, stream)`` of a reduction on ``device``: a tensor on that GPU and torch's current stream there
        (the ``_device`` entries, ordered after it); otherwise the host array, or the host copy of a tensor on another
        GPU, and ``None``."""
        if device != self.gpu:
            return self.host(), None
        import torch
        return self.data, torch.cuda.current_stream(self.data.device).cuda_stream

    def device_or_host(self, device, host: bool):
        """The ``device=`` argument of a measurement for a device class's ``device=`` / ``host=`` pair: the tensor's GPU
        unless another is named, or ``None`` (the host path) with ``host=True``."""
        if host:
            return None
        return self.gpu if device is None else device

    # -------------------------------------------------------------------------------------------------- segments
    def segment_table(self, segment_steps, hop, taper):
        """``(W, tau, starts)`` (``segment_plan``): the hop grid over a single run, or the segments of every run
        (``ensemble_segment_starts``), counted in frames of the joined series, none of them across a run boundary."""
        if self.run_lengths is None:
            width, hop, tau = segment_plan(self.frames, segment_steps, hop, taper)
            return width, tau, _segment_starts(self.frames, width, hop)
        width, hop, tau = segment_plan(min(self.run_lengths), segment_steps, hop, taper)
        return width, tau, ensemble_segment_starts(self.run_lengths, width, hop)[0]

    def whole_table(self, too_few=None):
        """The whole run as one boxcar segment, or each of several runs as one: those need one length.  ``too_few``: the
        message for fewer than three frames, where ``segment_plan``'s is not the caller's."""
        if self._whole_table is None:
            frames = self.frames if self.run_lengths is None else _equal_run_length(self.run_lengths)
            if too_few is not None and frames < 3:
                raise ValueError(too_few)
            self._whole_table = self.segment_table(frames, frames, "boxcar")
        return self._whole_table

    def segment_starts(self, segment_steps, hop=None):
        """What the classes' ``segment_starts`` return: the first frame of each segment of a single run, or
        ``(run_index, start_within_run)`` for runs."""
        if self.run_lengths is None:
            return self.segment_table(segment_steps, hop, "boxcar")[2]
        starts, run_index = ensemble_segment_starts(self.run_lengths, segment_steps, hop)
        return run_index, starts - _run_offsets(self.run_lengths)[run_index]


def _held(name: str, value, pattern, increments: bool = False) -> _Series:
    """The constructor argument of a host class: an array, checked here, or the holder a subclass has made."""
    if isinstance(value, _Series):
        return value
    verify_ndarray_shape(name, value, pattern)
    return _Series(value, increments=increments)


# ----------------------------------------------------------------------------- weight-contracted measurements
class _ContractedSpectrum:
    """``measure`` / ``measure_polarized`` of every spectrum that contracts the spectra of component pairs with weights
    (``polarized_weights``).  ``_whole(weights, device)`` returns the uncorrected ``(wavenumbers, I[K, *rows, bins])``
    and ``_row_axes`` counts the row axes between ``K`` and the bins: none for a whole spectrum, the ``G,G`` of the
    atom-group spectra, the ``C+1`` of the mode spectra.  The corrections apply to every row."""

    _row_axes = 0

    def _whole(self, weights, device):
        raise NotImplementedError

    def _first_configuration(self, intensities):
        """Drop the ``K`` axis, which stands before the rows."""
        return intensities[(..., 0) + (slice(None),) * (self._row_axes + 1)]

    def measure(self, orientation="polycrystalline", laser_correction=False, laser_wavelength=522,
                bose_einstein_correction=False, temperature=300, device=None):
        """``(wavenumbers, I[*rows, bins])`` of ``45 a^2 + 7 gamma^2``, the powder average."""
        _require_polycrystalline(orientation)
        wavenumbers, intensities = self._whole(_measure_weights(), device)
        intensities = _apply_corrections(wavenumbers, self._first_configuration(intensities), laser_correction,
                                         laser_wavelength, bose_einstein_correction, temperature)
        return wavenumbers, intensities

    def measure_polarized(self, incident, scattered, orientation=None, laser_correction=False, laser_wavelength=522,
                          bose_einstein_correction=False, temperature=300, device=None):
        """``(wavenumbers, I[K, *rows, bins])`` for the configurations of ``polarized_weights``; ``[*rows, bins]`` when
        no argument has a ``K`` axis."""
        weights, squeeze = polarized_weights(incident, scattered, orientation)
        wavenumbers, intensities = self._whole(weights, device)
        intensities = _apply_corrections(wavenumbers, intensities, laser_correction, laser_wavelength,
                                         bose_einstein_correction, temperature)
        return wavenumbers, self._first_configuration(intensities) if squeeze else intensities


class _ContractedMDSpectrum(_ContractedSpectrum):
    """The four weight-contracted measurements of the MD Raman classes (whole, atom-group, mode) over the series in
    ``self._series``.  A class supplies ``_reduce(weights, table, average, device)`` for a segment table
    ``(W, tau, starts)`` of the holder: the uncorrected ``(wavenumbers, I[K, *rows, bins])``, or
    ``I[Q, K, *rows, bins]`` with ``average=False``; ``device=None`` is the host path.  ``measure`` /
    ``measure_polarized`` take the holder's whole table, the segment measurements its segment table."""

    def __init__(self, series: _Series, timestep: float):
        self._series = series
        self._timestep = timestep

    @property
    def timestep(self) -> float:
        return self._timestep

    def _reduce(self, weights, table, average: bool, device):
        raise NotImplementedError

    def _whole_table(self):
        return self._series.whole_table()

    def _whole(self, weights, device):
        return self._reduce(weights, self._whole_table(), True, device)

    def _segments(self, weights, segment_steps, hop, taper, average, device):
        return self._reduce(weights, self._series.segment_table(segment_steps, hop, taper), bool(average), device)

    def segment_starts(self, segment_steps, hop=None) -> NDArray[np.int64]:
        """The first frame of each of the ``Q = (S - segment_steps) // hop + 1`` segments of ``measure_segments``: the
        time axis of a spectrogram (segment q covers frames ``starts[q] .. starts[q] + segment_steps - 1``; for
        increments, frame t is where increment t begins)."""
        return self._series.segment_starts(segment_steps, hop)

    def measure_segments(self, segment_steps, hop=None, taper="hann", average=True, orientation="polycrystalline",
                         laser_correction=False, laser_wavelength=522, bose_einstein_correction=False, temperature=300,
                         device=None):
        """Segment-averaged (Welch) or time-resolved spectra of ``measure()``'s ``45 a^2 + 7 gamma^2``: the series is
        cut into ``Q`` overlapping segments of ``segment_steps`` frames, ``hop`` frames apart (default
        ``segment_steps // 2``), whose ``segment_steps - 1`` differences are multiplied by ``taper``
        (``spectrum.segment_plan``; normalised to a mean square of one).  ``average=True`` returns
        ``(wavenumbers, I[*rows, bins])``, the arithmetic mean over the segments, whose variance falls with ``Q`` where a
        single periodogram's does not fall with the length of the series; ``average=False`` the rows
        ``(wavenumbers, I[Q, *rows, bins])``.  No further normalisation is applied: magnitudes scale with the segment
        length as ``measure()``'s scale with the series length, and the wavenumbers are those of a ``segment_steps``
        series.  The corrections apply to every row."""
        _require_polycrystalline(orientation)
        wavenumbers, intensities = self._segments(_measure_weights(), segment_steps, hop, taper, average, device)
        intensities = _apply_corrections(wavenumbers, self._first_configuration(intensities), laser_correction,
                                         laser_wavelength, bose_einstein_correction, temperature)
        return wavenumbers, intensities

    def measure_segments_polarized(self, incident, scattered, orientation=None, *, segment_steps, hop=None,
                                   taper="hann", average=True, laser_correction=False, laser_wavelength=522,
                                   bose_einstein_correction=False, temperature=300, device=None):
        """``measure_segments`` for the configurations of ``measure_polarized`` (``polarized_weights``): intensities
        ``(K, *rows, bins)``, or ``(Q, K, *rows, bins)`` with ``average=False``; the ``K`` axis is squeezed when no
        argument has one."""
        weights, squeeze = polarized_weights(incident, scattered, orientation)
        wavenumbers, intensities = self._segments(weights, segment_steps, hop, taper, average, device)
        intensities = _apply_corrections(wavenumbers, intensities, laser_correction, laser_wavelength,
                                         bose_einstein_correction, temperature)
        return wavenumbers, self._first_configuration(intensities) if squeeze else intensities


class _Ensemble:
    """What the classes of several runs add to their single-run class."""

    @property
    def run_lengths(self) -> list[int]:
        """Frames per run (for runs of increments, one more than the run's increments)."""
        return list(self._series.run_lengths)

    def segment_starts(self, segment_steps, hop=None) -> tuple[NDArray[np.int64], NDArray[np.int64]]:
        """``(run_index, start_within_run)`` of each row of ``measure_segments(..., average=False)``."""
        return self._series.segment_starts(segment_steps, hop)


class _OnDevice:
    """Mixin for a Raman class whose series stays in HBM as a contiguous float64 CUDA tensor: ``measure`` /
    ``measure_polarized`` / ``measure_segments`` / ``measure_segments_polarized`` reduce it on the tensor's GPU unless
    ``host=True``; another ``device`` gets the host copy, which is made on first use."""

    def measure(self, orientation="polycrystalline", laser_correction=False, laser_wavelength=522,
                bose_einstein_correction=False, temperature=300, device=None, host=False):
        """As the base class's ``measure``; reduces on the tensor's GPU unless ``host=True``."""
        return super().measure(orientation, laser_correction, laser_wavelength, bose_einstein_correction,
                               temperature, device=self._series.device_or_host(device, host))

    def measure_polarized(self, incident, scattered, orientation=None, laser_correction=False,
                          laser_wavelength=522, bose_einstein_correction=False, temperature=300, device=None,
                          host=False):
        """As the base class's ``measure_polarized``; reduces on the tensor's GPU unless ``host=True`` (the
        ``_device`` entries: only the intensities leave HBM)."""
        return super().measure_polarized(incident, scattered, orientation, laser_correction, laser_wavelength,
                                         bose_einstein_correction, temperature,
                                         device=self._series.device_or_host(device, host))

    def measure_segments(self, segment_steps, hop=None, taper="hann", average=True, orientation="polycrystalline",
                         laser_correction=False, laser_wavelength=522, bose_einstein_correction=False, temperature=300,
                         device=None, host=False):
        """As the base class's ``measure_segments``; reduces on the tensor's GPU unless ``host=True``."""
        return super().measure_segments(segment_steps, hop, taper, average, orientation, laser_correction,
                                        laser_wavelength, bose_einstein_correction, temperature,
                                        device=self._series.device_or_host(device, host))

    def measure_segments_polarized(self, incident, scattered, orientation=None, *, segment_steps, hop=None,
                                   taper="hann", average=True, laser_correction=False, laser_wavelength=522,
                                   bose_einstein_correction=False, temperature=300, device=None, host=False):
        """As the base class's ``measure_segments_polarized``; reduces on the tensor's GPU unless ``host=True``."""
        return super().measure_segments_polarized(
            incident, scattered, orientation, segment_steps=segment_steps, hop=hop, taper=taper, average=average,
            laser_correction=laser_correction, laser_wavelength=laser_wavelength,
            bose_einstein_correction=bose_einstein_correction, temperature=temperature,
            device=self._series.device_or_host(device, host))


# ----------------------------------------------------------------------------- the whole MD spectrum
class MDRamanSpectrum(_ContractedMDSpectrum, RamanSpectrum):
    """Spectrum from a polarizability time series ``(S,3,3)`` and a timestep in fs
    (``spectrum/_raman.py:197-309``).

    ``measure_polarized``: spectra for set incident / scattered polarizations and crystal orientations (an addition).
    Configuration k's spectrum is ``calc_signal_spectrum(s_k, timestep)`` without the zero bin, on ``measure``'s
    wavenumbers, for ``s_k(t) = e_s . R da(t) R^T . e_i`` with ``da(t) = alpha(t+1) - alpha(t)``; the symmetric part of
    ``da`` is used (every model output is exactly symmetric).  Arguments as ``PhononRamanSpectrum.measure_polarized``;
    under ``"polycrystalline"`` the invariant spectra take the place of ``a^2`` and ``gamma^2``, so
    ``45 (I_parallel + I_perpendicular)`` is ``measure()``.  Intensities are ``(K, bins)``, or ``(bins,)`` when no
    argument has a ``K`` axis.  The 21 cross-spectra of the tensor components are computed once and contracted with each
    configuration's weights (``polarized_weights``); ``device`` (an int) does that on the GPU
    (``rn_md_raman_polarized``).

    ``measure_segments`` (an addition) is the segment-averaged (Welch) or time-resolved spectrum of ``measure()``:
    ``(wavenumbers, I[bins])``, or with ``average=False`` the spectrogram ``(wavenumbers, I[Q, bins])``.  Row q is the
    spectrum of segment q: with ``taper="boxcar"`` it is
    ``MDRamanSpectrum(alpha[a:a + segment_steps], timestep).measure()`` for ``a = segment_starts(...)[q]``.  ``device``
    (an int) reduces on that GPU (``rn_md_raman_segments``: the mean is taken before the inverse transform).
    ``measure_segments_polarized`` returns ``(K, bins)``, or ``(Q, K, bins)`` with ``average=False``."""

    def __init__(self, polarizability_ts, timestep: float):
        super().__init__(_held("polarizability_ts", polarizability_ts, (None, 3, 3)), timestep)

    @property
    def polarizability_ts(self):
        return self._series.host()

    def measure(self, orientation="polycrystalline", laser_correction=False,
                laser_wavelength=522, bose_einstein_correction=False, temperature=300, device=None):
        """``device`` (an int, not in the reference's signature): reduce the time series on that
        GPU (``rn_md_raman_intensities``: one batched FFT, one power spectrum, two more FFTs)
        instead of on the host; pays off for very long series (S >> 1e5) or many models."""
        _require_polycrystalline(orientation)
        dt = self._timestep
        if device is not None:
            source, stream = self._series.source(int(device))
            wavenumbers, intensities = _md_intensities_on_device(source, dt, int(device), stream)
            intensities = _apply_corrections(wavenumbers, intensities, laser_correction,
                                             laser_wavelength, bose_einstein_correction, temperature)
            return wavenumbers, intensities
        ad = np.diff(self._series.host(), axis=0)  # d(alpha)/dt up to a constant

        def spec(sig):
            return calc_signal_spectrum(sig, dt)[1]

        wavenumbers, _ = calc_signal_spectrum(ad[:, 0, 0], dt)
        alpha2 = (1 / 9) * spec(ad[:, 0, 0] + ad[:, 1, 1] + ad[:, 2, 2])
        gamma2 = (
            (1 / 2) * spec(ad[:, 0, 0] - ad[:, 1, 1])
            + (1 / 2) * spec(ad[:, 1, 1] - ad[:, 2, 2])
            + (1 / 2) * spec(ad[:, 2, 2] - ad[:, 0, 0])
            + 3 * spec(ad[:, 0, 1]) + 3 * spec(ad[:, 1, 2]) + 3 * spec(ad[:, 0, 2])
        )
        intensities = (45.0 * alpha2 + 7.0 * gamma2)[1:]  # the 0 cm^-1 bin is dropped
        wavenumbers = wavenumbers[1:]
        intensities = _apply_corrections(wavenumbers, intensities, laser_correction,
                                         laser_wavelength, bose_einstein_correction, temperature)
        return wavenumbers, intensities

    def _whole(self, weights, device):
        """A single run has entries of its own: the 21 cross-spectra of the whole series."""
        if device is not None:
            source, stream = self._series.source(int(device))
            return _md_polarized_on_device(source, self._timestep, weights, int(device), stream=stream)
        wavenumbers, basis = _md_basis_spectra(np.asarray(self._series.host(), dtype=np.float64), self._timestep)
        return wavenumbers, weights @ basis

    def _segments(self, weights, segment_steps, hop, taper, average, device):
        """A single run goes to the hop-grid entry (``rn_md_raman_segments``), which builds the table itself."""
        width, hop, tau = segment_plan(self._series.frames, segment_steps, hop, taper)
        if device is None:
            return _md_segments_host(self._series.host(), self._timestep, weights, width, hop, tau, bool(average))
        source, stream = self._series.source(int(device))
        return _md_segments_on_device(source, self._timestep, weights, width, hop, tau, bool(average), int(device),
                                      stream=stream)

    def _reduce(self, weights, table, average: bool, device):
        width, tau, starts = table
        if device is None:
            return _md_segments_host(self._series.host(), self._timestep, weights, width, None, tau, bool(average),
                                     starts=starts)
        source, stream = self._series.source(int(device))
        return _md_segments_at_on_device(source, self._timestep, weights, width, starts, tau, bool(average), int(device),
                                         stream=stream)


class DeviceMDRamanSpectrum(_OnDevice, MDRamanSpectrum):
    """``MDRamanSpectrum`` whose polarizability time series stays where the evaluator wrote it
    (HBM, a contiguous torch CUDA tensor ``float64[S,3,3]``): ``measure`` reduces it on that GPU
    and only the intensities travel to the host.  ``polarizability_ts``
    copies the series to the host on first use, for callers that want the numbers themselves."""

    def __init__(self, polarizability_ts_device, timestep: float):
        super().__init__(_Series.of_tensor("polarizability_ts", polarizability_ts_device, (None, 3, 3)), timestep)

    @property
    def _device_ts(self):
        return self._series.data


class MDRamanEnsemble(_Ensemble, MDRamanSpectrum):
    """Spectra averaged over several independent runs (an addition): ``runs`` is a sequence of polarizability time
    series ``(S_r,3,3)`` sharing ``timestep`` (fs), for example NVE branches started from NVT snapshots.

    ``measure_segments`` / ``measure_segments_polarized`` are ``MDRamanSpectrum``'s with the segments of every run
    (``ensemble_segment_starts``): ``average=True`` is the mean over all segments of all runs, ``average=False`` gives
    the rows in run order.  No segment crosses a run boundary, where the difference of the joined series is a jump
    that would put a broadband artefact into every bin.  ``measure`` / ``measure_polarized`` are the mean of the runs'
    whole spectra (the boxcar segment of ``S_r`` steps), defined when the runs have one length: ``measure`` is the mean
    of ``MDRamanSpectrum(run, timestep).measure()`` over the runs and ``measure_polarized`` that of the runs'
    ``measure_polarized``; a ``ValueError`` unless they have one length (their wavenumbers differ otherwise).
    ``device`` (an int) reduces all runs in one call on that GPU (``rn_md_raman_segments_at``)."""

    # runs have no entry of a single series: every measurement is the base's, over the holder's tables
    measure = _ContractedMDSpectrum.measure
    _whole = _ContractedMDSpectrum._whole
    _segments = _ContractedMDSpectrum._segments

    def __init__(self, runs, timestep: float):
        super().__init__(runs if isinstance(runs, _Series) else _Series.of_runs(runs, (3, 3), False), timestep)

    @property
    def runs(self):
        """The runs' series, views of the joined ``polarizability_ts``."""
        bounds = np.cumsum(self._series.run_lengths)[:-1]
        return np.split(self._series.host(), bounds, axis=0)


class DeviceMDRamanEnsemble(_OnDevice, MDRamanEnsemble):
    """``MDRamanEnsemble`` whose runs stay in HBM: ``runs`` is a sequence of contiguous float64 CUDA tensors
    ``(S_r,3,3)`` (joined here, on the GPU), or one tensor holding them end to end plus ``run_lengths``, as one batched
    evaluation writes it.  Every measurement reduces on that GPU (``rn_md_raman_segments_at_device``, ordered after
    torch's current stream) unless ``host=True``."""

    def __init__(self, runs, timestep: float, run_lengths=None):
        super().__init__(_Series.of_tensor_runs("runs", runs, run_lengths, (None, 3, 3)), timestep)


# ----------------------------------------------------------------------------- atom-group (partial) spectra
MAX_GROUPS = 16  # kMaxGroups of csrc/kernels.hpp


def group_labels(groups, atomic_numbers) -> tuple[NDArray[np.int32], int]:
    """Resolve ``groups`` for a structure with ``atomic_numbers`` ``(N,)`` into ``(labels int32[N], G)``.

    ``groups`` is an integer array ``(N,)`` of labels in ``[0, G)``, every label used, ``1 <= G <= 16``; or
    ``"species"``: one group per distinct atomic number, in ascending atomic number.  Anything else (a wrong length, a
    negative or non-integer label, an empty group, ``G > 16``, another string) is a ``ValueError``.  Every partial
    spectrum path resolves its groups here."""
    numbers = np.asarray(atomic_numbers)
    n = numbers.shape[0]
    if isinstance(groups, str):
        if groups != "species":
            raise ValueError(f"unknown groups: {groups!r} (an integer array (N,) or 'species')")
        species, labels = np.unique(numbers, return_inverse=True)
        labels = labels.reshape(-1)
        count = len(species)
    else:
        if groups is None or isinstance(groups, bytes):
            raise ValueError("groups must be an integer array (N,) or 'species'")
        labels = np.asarray(groups)
        if labels.dtype.kind not in "iu":
            raise ValueError(f"groups must hold integer labels, not {labels.dtype}")
        if labels.shape != (n,):
            raise ValueError(f"groups has wrong shape: {shape_string(labels.shape)} != ({n},)")
        if n and labels.min() < 0:
            raise ValueError("groups holds a negative label")
        count = int(labels.max()) + 1 if n else 0
        used = np.bincount(labels.astype(np.int64), minlength=count)
        if count and np.any(used == 0):
            raise ValueError(f"groups leaves group(s) {np.flatnonzero(used == 0).tolist()} empty")
    if count < 1:
        raise ValueError("groups defines no group")
    if count > MAX_GROUPS:
        raise ValueError(f"groups defines {count} groups, more than {MAX_GROUPS}")
    return np.ascontiguousarray(labels, dtype=np.int32), count


def _weight_forms(weights: NDArray[np.float64]) -> NDArray[np.float64]:
    """``W[K][21]`` -> the symmetric 6x6 forms ``M[K]`` (off-diagonal entries halved back)."""
    forms = np.zeros((weights.shape[0], 6, 6))
    forms[:, _PAIR_J, _PAIR_L] = weights / _PAIR_SCALE
    forms[:, _PAIR_L, _PAIR_J] = weights / _PAIR_SCALE
    return forms


def _measure_weights() -> NDArray[np.float64]:
    """The weights of ``measure()`` (``45 a^2 + 7 gamma^2``): 45 (parallel + perpendicular) of the powder average."""
    weights, _ = polarized_weights([1.0, 0.0, 0.0], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], "polycrystalline")
    return 45.0 * weights.sum(axis=0, keepdims=True)


def _unpack_pairs(packed: NDArray[np.float64], num_groups: int) -> NDArray[np.float64]:
    """``[K][G(G+1)/2][bins]`` (pairs g <= h, row-major) -> the symmetric ``[K,G,G,bins]``."""
    rows, cols = np.triu_indices(num_groups)
    out = np.empty((packed.shape[0], num_groups, num_groups, packed.shape[-1]))
    out[:, rows, cols] = packed
    out[:, cols, rows] = packed
    return out


def _md_partial_host(increments: NDArray[np.float64], timestep: float, weights: NDArray[np.float64]):
    """(wavenumbers, ``I[K,G,G,bins]``) on the host: for each pair of groups, calc_signal_spectrum's transform of the
    symmetrised cross-correlation of their component series, contracted with each configuration's form, zero bin
    dropped (``include/rn_potgnn.h``, ``rn_md_raman_partial``)."""
    d = _symmetric_components(np.asarray(increments, dtype=np.float64))  # (N, G, 6)
    n, num_groups = d.shape[:2]
    wavenumbers, keep, length = _lag_axis(n, timestep)
    spectra = np.fft.rfft(d, n=length, axis=0)  # (length / 2 + 1, G, 6)
    forms = _weight_forms(weights)
    out = np.empty((weights.shape[0], num_groups, num_groups, len(keep)))
    for g in range(num_groups):
        for h in range(g, num_groups):
            cross = np.real(spectra[:, g, :, None] * np.conj(spectra[:, h, None, :]))
            power = np.einsum("kce,fce->kf", forms, cross)
            out[:, g, h] = out[:, h, g] = _lag_spectrum(power, n, length, keep)
    return wavenumbers, out


def _md_partial_on_device(increments, timestep: float, weights, device: int, stream=None, workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K,G,G,bins]``) from ``rn_md_raman_partial`` (host increments) or, with a torch CUDA
    tensor, ``rn_md_raman_partial_device`` ordered after ``stream``."""
    n, num_groups = increments.shape[0], increments.shape[1]
    weights, weight_args = _weights_arguments(weights)
    wavenumbers, packed = _call_md_reducer(
        "rn_md_raman_partial", increments, n, "the device reduction needs at least two increments", timestep, device,
        stream, (weights.shape[0], num_groups * (num_groups + 1) // 2), (n, num_groups, *weight_args), (workspace_limit,))
    return wavenumbers, _unpack_pairs(packed, num_groups)


def _md_partial_segments_host(increments, timestep: float, weights, width: int, starts, tau, average: bool):
    """(wavenumbers, ``I[K,G,G,bins]`` or ``I[Q,K,G,G,bins]``) on the host, from the definition (``include/rn_potgnn.h``,
    ``rn_md_raman_partial_segments``): per segment of ``width`` frames starting at frame ``starts[q]`` the zero-padded
    transforms of the tapered components of increments ``starts[q] .. starts[q] + width - 2``, for each pair of groups
    their cross-power contracted with each configuration's form, its inverse transform, the positive lags and their
    length-n transform; the mean over the segments is taken on the contracted cross-powers."""
    d = _symmetric_components(np.asarray(increments, dtype=np.float64))  # (N, G, 6)
    num_groups = d.shape[1]
    n = width - 1
    starts = np.asarray(starts, dtype=np.int64)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    forms = _weight_forms(weights)
    count = weights.shape[0]
    rows, cols = np.triu_indices(num_groups)

    out = None if average else np.empty((len(starts), count, len(rows), len(keep)))
    mean = np.zeros((count, len(rows), length // 2 + 1))
    per_segment = (length // 2 + 1) * max(6 * num_groups, 36, count)
    chunk = max(1, _SEGMENT_CHUNK_ELEMENTS // per_segment)
    for first in range(0, len(starts), chunk):
        index = starts[first:first + chunk, None] + np.arange(n)[None, :]
        spectra = np.fft.rfft(d[index] * tau[None, :, None, None], n=length, axis=1)  # (q, length / 2 + 1, G, 6)
        for pair, (g, h) in enumerate(zip(rows, cols)):
            cross = np.real(spectra[:, :, g, :, None] * np.conj(spectra[:, :, h, None, :]))
            power = np.einsum("kce,qfce->qkf", forms, cross)
            if average:
                mean[:, pair] += power.sum(axis=0)
            else:
                out[first:first + chunk, :, pair] = _lag_spectrum(power, n, length, keep)
    if average:
        return wavenumbers, _unpack_pairs(_lag_spectrum(mean / len(starts), n, length, keep), num_groups)
    unpacked = _unpack_pairs(out.reshape(len(starts) * count, len(rows), len(keep)), num_groups)
    return wavenumbers, unpacked.reshape(len(starts), count, num_groups, num_groups, len(keep))


def _md_partial_segments_on_device(increments, timestep: float, weights, width: int, starts, tau, average: bool,
                                   device: int, stream=None, workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K,G,G,bins]`` or ``I[Q,K,G,G,bins]``) from ``rn_md_raman_partial_segments`` (host
    increments) or, with a torch CUDA tensor, ``rn_md_raman_partial_segments_device`` ordered after ``stream``."""
    import ctypes as C
    steps, num_groups = increments.shape[0], increments.shape[1]
    pairs = num_groups * (num_groups + 1) // 2
    weights, weight_args = _weights_arguments(weights)
    starts, table_args = _table_arguments(starts)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    count = weights.shape[0]
    shape = (count, pairs) if average else (len(starts) * count, pairs)
    wavenumbers, packed = _call_md_reducer(
        "rn_md_raman_partial_segments", increments, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
        (steps, num_groups, width, *table_args, C.c_void_p(tau.ctypes.data), *weight_args, int(bool(average))),
        (workspace_limit,))
    unpacked = _unpack_pairs(packed, num_groups)
    if not average:
        unpacked = unpacked.reshape(len(starts), count, num_groups, num_groups, -1)
    return wavenumbers, unpacked


class PartialPhononRamanSpectrum(_ContractedSpectrum):
    """Atom-group decomposition of a phonon spectrum: wavenumbers ``(M,)`` and partial Raman tensors ``(M,G,3,3)``
    (``R[m,g] = 2 sum_{i in g} J_i . d_{m,i}``, ``PotGNN.calc_partial_raman_tensors``).  ``I[g,h](m)`` is the bilinear
    form of the chosen intensity between ``R[m,g]`` and ``R[m,h]``: ``sum_{g,h}`` is the spectrum of ``sum_g R[m,g]``, and
    ``I[g,g]`` that of group g's tensors alone (the reference's masking of the other atoms' displacements).

    ``measure`` returns ``(wavenumbers, I[G,G,M])``: ``I[g,h]`` is the symmetric bilinear form of ``measure()``'s
    ``45 a^2 + 7 gamma^2`` between groups g and h, so ``I.sum((0, 1))`` is the whole spectrum and ``I[g,g]`` the
    spectrum of group g alone.  ``measure_polarized`` returns ``(wavenumbers, I[K,G,G,M])`` for the configurations of
    ``polarized_weights``; ``[G,G,M]`` when no argument has a ``K`` axis, as ``measure_polarized`` squeezes.  The
    corrections apply to every ``(g, h)`` row."""

    _row_axes = 2

    def __init__(self, phonon_wavenumbers, partial_raman_tensors) -> None:
        verify_ndarray_shape("phonon_wavenumbers", phonon_wavenumbers, (None,))
        verify_ndarray_shape("partial_raman_tensors", partial_raman_tensors, (len(phonon_wavenumbers), None, 3, 3))
        self._phonon_wavenumbers = phonon_wavenumbers
        self._partial_raman_tensors = partial_raman_tensors

    @property
    def phonon_wavenumbers(self):
        return self._phonon_wavenumbers.copy()

    @property
    def partial_raman_tensors(self):
        return self._partial_raman_tensors.copy()

    def _whole(self, weights, device):
        del device  # (at most 3N modes: always the host)
        d = _symmetric_components(np.asarray(self._partial_raman_tensors, dtype=np.float64))  # (M, G, 6)
        intensities = np.einsum("kce,mgc,mhe->kghm", _weight_forms(weights), d, d)
        rows, cols = np.triu_indices(d.shape[1], 1)
        intensities[:, cols, rows] = intensities[:, rows, cols]  # (exactly symmetric)
        return self._phonon_wavenumbers, intensities


class PartialMDRamanSpectrum(_ContractedMDSpectrum):
    """Atom-group decomposition of an MD spectrum: per-group polarizability increments ``(S-1,G,3,3)``
    (``PotGNN.calc_group_increments``) and a timestep in fs.  ``I[g,h]`` is the transform of the symmetrised
    cross-correlation of groups g and h, so ``I[g,g]`` is ``MDRamanSpectrum(cumsum of group g's increments).measure()`` and
    ``sum_{g,h} I`` that of the summed increments.  ``device`` (an int) reduces on that GPU (``rn_md_raman_partial``).

    ``measure`` returns ``(wavenumbers, I[G,G,bins])``: ``I[g,h]`` is the symmetric bilinear form of ``measure()``'s
    ``45 a^2 + 7 gamma^2`` between groups g and h, so ``I.sum((0, 1))`` is the whole spectrum and ``I[g,g]`` the
    spectrum of group g alone.  ``measure_polarized`` returns ``(wavenumbers, I[K,G,G,bins])`` for the configurations of
    ``polarized_weights``; ``[G,G,bins]`` when no argument has a ``K`` axis, as ``measure_polarized`` squeezes.  The
    corrections apply to every ``(g, h)`` row.

    ``measure_segments``: segment-averaged (Welch) or time-resolved partial spectra over
    ``MDRamanSpectrum.measure_segments``' segments of ``segment_steps`` frames (``segment_steps - 1`` increments each),
    with ``I[g,h]`` of ``measure()`` per segment.  ``average=True`` returns ``(wavenumbers, I[G,G,bins])``, the mean over
    the segments, whose variance falls with their number; ``average=False`` the rows ``(wavenumbers, I[Q,G,G,bins])``.
    With ``taper="boxcar"`` row q is ``PartialMDRamanSpectrum(increments[a:a + segment_steps - 1], timestep).measure()``
    for ``a = segment_starts(...)[q]``, the first frame of the segment (frame t is where increment t begins).
    ``device`` (an int) reduces on that GPU (``rn_md_raman_partial_segments``).  ``measure_segments_polarized`` returns
    ``I[K,G,G,bins]``, or ``I[Q,K,G,G,bins]`` with ``average=False``; the ``K`` axis is squeezed when no argument has
    one."""

    _row_axes = 2

    def __init__(self, increments, timestep: float):
        super().__init__(_held("increments", increments, (None, None, 3, 3), increments=True), timestep)

    @property
    def increments(self):
        return self._series.host()

    def _whole(self, weights, device):
        """A single run has an entry of its own (``rn_md_raman_partial``)."""
        if device is None:
            return _md_partial_host(self._series.host(), self._timestep, weights)
        source, stream = self._series.source(int(device))
        return _md_partial_on_device(source, self._timestep, weights, int(device), stream=stream)

    def _reduce(self, weights, table, average: bool, device):
        width, tau, starts = table
        if device is None:
            return _md_partial_segments_host(self._series.host(), self._timestep, weights, width, starts, tau,
                                             bool(average))
        source, stream = self._series.source(int(device))
        return _md_partial_segments_on_device(source, self._timestep, weights, width, starts, tau, bool(average),
                                              int(device), stream=stream)


class DevicePartialMDRamanSpectrum(_OnDevice, PartialMDRamanSpectrum):
    """``PartialMDRamanSpectrum`` whose increments stay in HBM (a contiguous float64 CUDA tensor ``(S-1,G,3,3)``):
    ``measure`` / ``measure_polarized`` and the segment measurements reduce them on that GPU
    (``rn_md_raman_partial_device``, ``rn_md_raman_partial_segments_device``, ordered after torch's current stream)
    unless ``host=True``; ``increments`` copies them to the host on first use."""

    def __init__(self, increments_device, timestep: float):
        super().__init__(_Series.of_tensor("increments", increments_device, (None, None, 3, 3), increments=True),
                         timestep)


class PartialMDRamanEnsemble(_Ensemble, PartialMDRamanSpectrum):
    """Atom-group spectra averaged over several runs: ``runs`` is a sequence of per-group increments ``(S_r-1,G,3,3)``
    sharing ``G`` and ``timestep``.  The runs are joined with one zero row between them, so that increment t still
    belongs to frame t of the joined frames; no segment reads that row.  ``measure_segments`` /
    ``measure_segments_polarized`` take the segments of every run (``ensemble_segment_starts`` of the runs' ``S_r``
    frames; rows in run order, ``average=True`` the mean over all of them), ``measure`` / ``measure_polarized`` the mean
    of the runs' whole spectra when the runs have one length: one boxcar segment per run.  ``device`` (an int) reduces
    all runs in one call (``rn_md_raman_partial_segments``)."""

    _whole = _ContractedMDSpectrum._whole  # runs have no entry of a single series

    def __init__(self, runs, timestep: float):
        super().__init__(runs if isinstance(runs, _Series) else _Series.of_runs(runs, (3, 3), True, increments=True),
                         timestep)


class DevicePartialMDRamanEnsemble(_OnDevice, PartialMDRamanEnsemble):
    """``PartialMDRamanEnsemble`` whose increments stay in HBM: a sequence of contiguous float64 CUDA tensors
    ``(S_r-1,G,3,3)`` (joined here, on the GPU, with a zero row between them), or one tensor ``(sum(S_r)-1,G,3,3)``
    plus ``run_lengths`` (frames per run), as one batched evaluation of the joined frames writes it: its rows across
    the run boundaries stand where the zero rows would and are never read."""

    def __init__(self, runs, timestep: float, run_lengths=None):
        super().__init__(_Series.of_tensor_runs("runs", runs, run_lengths, (None, None, 3, 3), increments=True),
                         timestep)


# ----------------------------------------------------------------------------- vibrational density of states
def _vdos_lattices(lattice, frames: int) -> NDArray[np.float64]:
    """``lattice`` ``(3,3)`` (a fixed cell) or ``(frames,3,3)`` (a lattice per frame) as float64 ``(1 or frames,3,3)``,
    rows = lattice vectors in Angstrom; ``ValueError`` on another shape, a non-finite entry or a singular lattice
    (``dynamics.verify_lattices``)."""
    from ramannoodle_amd.dynamics import verify_lattices
    if lattice is None or isinstance(lattice, (str, bytes)):
        raise get_type_error("lattice", lattice, "ndarray")
    array = np.asarray(lattice)
    if array.shape == (3, 3):
        return verify_lattices(array[None], 1)
    if array.ndim != 3:
        raise ValueError(f"lattice has wrong shape: {shape_string(array.shape)} != (3,3) or ({frames},3,3)")
    return verify_lattices(array, frames)


def _vdos_masses(masses, atoms: int) -> NDArray[np.float64]:
    """``masses`` ``(atoms,)``, finite and positive, as float64; ``None``: unit masses."""
    if masses is None:
        return np.ones(atoms)
    if isinstance(masses, (str, bytes)):
        raise get_type_error("masses", masses, "ndarray")
    array = np.asarray(masses)
    if array.dtype.kind not in "iuf":
        raise get_type_error("masses", masses, "ndarray of real numbers")
    if array.shape != (atoms,):
        raise ValueError(f"masses has wrong shape: {shape_string(array.shape)} != ({atoms},)")
    array = np.ascontiguousarray(array, dtype=np.float64)
    if not (np.all(np.isfinite(array)) and np.all(array > 0)):
        raise ValueError("masses must be finite and positive")
    return array


def _vdos_labels(labels, num_groups, atoms: int) -> tuple[NDArray[np.int32], int]:
    """``labels`` ``(atoms,)`` in ``[0, num_groups)``, ``1 <= num_groups <= 16``, as int32; ``None``: one group."""
    if isinstance(num_groups, (bool, np.bool_)) or not isinstance(num_groups, (int, np.integer)):
        raise get_type_error("num_groups", num_groups, "int")
    count = int(num_groups)
    if not 1 <= count <= MAX_GROUPS:
        raise ValueError(f"invalid num_groups: {count} is not in [1, {MAX_GROUPS}]")
    if labels is None:
        if count != 1:
            raise ValueError(f"num_groups = {count} needs labels")
        return np.zeros(atoms, dtype=np.int32), 1
    array = np.asarray(labels)
    if array.dtype.kind not in "iu":
        raise ValueError(f"labels must hold integers, not {array.dtype}")
    if array.shape != (atoms,):
        raise ValueError(f"labels has wrong shape: {shape_string(array.shape)} != ({atoms},)")
    if atoms and (array.min() < 0 or array.max() >= count):
        raise ValueError(f"labels must lie in [0, {count})")
    return np.ascontiguousarray(array, dtype=np.int32), count


def _vdos_steps(positions: NDArray[np.float64], lattices: NDArray[np.float64]) -> NDArray[np.float64]:
    """The Cartesian minimum-image steps ``u[t] = (df - rint(df)) @ M[t]``, ``df = f[t+1] - f[t]``: ``(S-1,N,3)``.
    ``M[t]`` is the one lattice, or the midpoint ``(Lat[t] + Lat[t+1]) / 2`` of a lattice per frame."""
    steps = np.diff(positions, axis=0)
    steps -= np.rint(steps)
    if lattices.shape[0] == 1:
        return steps @ lattices[0]
    return np.einsum("tik,tkc->tic", steps, 0.5 * (lattices[:-1] + lattices[1:]))


def _vdos_host(positions, lattices, masses, labels, num_groups: int, timestep: float, width: int, starts, tau,
               average: bool):
    """(wavenumbers, ``D[G][bins]`` or ``D[Q][G][bins]``) on the host, from the definition (``include/rn_potgnn.h``,
    ``rn_md_vdos``): per segment the zero-padded transforms of the tapered, mass-weighted minimum-image steps of every
    atom and direction, their power summed per group, its inverse transform, the positive lags and their length-n
    transform; the mean over the segments is taken on the group powers.  Only the steps of the segments are read."""
    u = _vdos_steps(np.asarray(positions, dtype=np.float64), lattices) * np.sqrt(masses)[None, :, None]
    n = width - 1
    starts = np.asarray(starts, dtype=np.int64)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    atoms = u.shape[1]
    members = [np.flatnonzero(labels == g) for g in range(num_groups)]

    rows = None if average else np.empty((len(starts), num_groups, len(keep)))
    mean = np.zeros((num_groups, length // 2 + 1))
    chunk = max(1, _SEGMENT_CHUNK_ELEMENTS // (3 * (length // 2 + 1)))
    for q, start in enumerate(starts):
        atom_power = np.empty((atoms, length // 2 + 1))
        for first in range(0, atoms, chunk):
            series = u[start:start + n, first:first + chunk] * tau[:, None, None]
            spectra = np.fft.rfft(series, n=length, axis=0)  # (length / 2 + 1, atoms of the chunk, 3)
            atom_power[first:first + chunk] = (spectra.real ** 2 + spectra.imag ** 2).sum(axis=2).T
        power = np.stack([atom_power[index].sum(axis=0) for index in members])
        if average:
            mean += power
        else:
            rows[q] = _lag_spectrum(power, n, length, keep)
    return wavenumbers, _lag_spectrum(mean / len(starts), n, length, keep) if average else rows


def _step_reducer_on_device(entry: str, positions, lattices, masses, rows, count: int, timestep: float, width: int,
                            starts, tau, average: bool, device: int, stream, workspace_limit: int):
    """What ``rn_md_vdos`` and ``rn_md_mode_vdos`` share, argument for argument: ``rows`` is the reducer's own array, already
    contiguous and typed (the labels; the vectors), ``count`` the number of rows it yields per segment (G; M).  Host
    positions and lattices, or two torch CUDA tensors and the ``_device`` entry ordered after ``stream``."""
    import ctypes as C
    steps, atoms = int(positions.shape[0]), int(positions.shape[1])
    if stream is None:
        lattices = np.ascontiguousarray(lattices, dtype=np.float64)
        lattice_pointer = lattices.ctypes.data
    else:
        lattice_pointer = lattices.data_ptr()
    masses = np.ascontiguousarray(masses, dtype=np.float64)
    starts, table_args = _table_arguments(starts)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    shape = (count,) if average else (len(starts), count)
    return _call_md_reducer(
        entry, positions, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
        (C.c_void_p(lattice_pointer), int(lattices.shape[0]), steps, atoms, C.c_void_p(masses.ctypes.data),
         C.c_void_p(rows.ctypes.data), count, width, *table_args, C.c_void_p(tau.ctypes.data), int(bool(average))),
        (workspace_limit,))


def _vdos_on_device(positions, lattices, masses, labels, num_groups: int, timestep: float, width: int, starts, tau,
                    average: bool, device: int, stream=None, workspace_limit: int = 0):
    """(wavenumbers, ``D[G][bins]`` or ``D[Q][G][bins]``) from ``rn_md_vdos`` (host positions and lattices) or, with two
    torch CUDA tensors, ``rn_md_vdos_device`` ordered after ``stream``."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    return _step_reducer_on_device("rn_md_vdos", positions, lattices, masses, labels, num_groups, timestep, width,
                                   starts, tau, average, device, stream, workspace_limit)


def _lattice_on_device(lattice, positions):
    """``(lattice for _vdos_lattices, lattice CUDA tensor or None)`` of positions in HBM: a lattice per frame that is a
    CUDA tensor is reduced from where it is; any other is made from the validated host lattices on first use."""
    import torch
    if not isinstance(lattice, torch.Tensor):
        return lattice, None
    host_lattice = lattice.detach().cpu().numpy()
    if not (lattice.is_cuda and lattice.ndim == 3):
        return host_lattice, None
    if not (lattice.is_contiguous() and lattice.dtype == torch.float64 and lattice.device == positions.device):
        raise ValueError("lattice must be a contiguous float64 CUDA tensor on the positions' GPU")
    return host_lattice, lattice


class VibrationalDensityOfStates:
    """Vibrational density of states (VDOS) of an MD run, whole and by atom group (an addition): which vibrations exist
    at all, on the wavenumber axis of ``MDRamanSpectrum`` for the same number of frames and timestep, so that the two
    curves overlay bin for bin.

    ``positions_ts``: fractional positions ``(S,N,3)``, wrapped into the cell or not; ``timestep`` in fs; ``lattice``:
    ``(3,3)`` (a fixed cell) or ``(S,3,3)`` (a lattice per frame), rows = lattice vectors in Angstrom; ``masses``
    ``(N,)``, finite and positive (``None``: unit masses); ``labels`` ``(N,)`` integers in ``[0, num_groups)``,
    ``1 <= num_groups <= 16`` (``None``: one group).

    The step of atom i from frame t to t + 1 is the minimum image ``df - rint(df)`` of ``df = f[t+1] - f[t]`` taken to
    Cartesian coordinates by the lattice (a lattice per frame: by the midpoint ``(Lat[t] + Lat[t+1]) / 2``, the motion
    relative to the deforming cell), not divided by the timestep.  ``D[g]`` is the sum over the atoms of group g and the
    three directions of ``calc_signal_spectrum(sqrt(m_i) u_i,c)`` without the zero bin, so ``D.sum(0)`` is the one-group
    VDOS and magnitudes scale with the series length as ``MDRamanSpectrum.measure``'s do.  ``device`` (an int) reduces on
    that GPU (``rn_md_vdos``); ``None`` is the host path."""

    def __init__(self, positions_ts, timestep: float, lattice, masses=None, labels=None, num_groups=1):
        if isinstance(positions_ts, _Series):  # (a subclass's holder)
            self._series = positions_ts
        else:
            verify_ndarray_shape("positions_ts", positions_ts, (None, None, 3))
            self._series = _Series(np.ascontiguousarray(positions_ts, dtype=np.float64))
        self._lattice_tensor = None  # the lattices beside a series in HBM
        if self._series.gpu is not None:
            lattice, self._lattice_tensor = _lattice_on_device(lattice, self._series.data)
        steps, atoms = (int(size) for size in self._series.shape[:2])
        self._timestep = timestep
        self._lattices = _vdos_lattices(lattice, steps)
        self._masses = _vdos_masses(masses, atoms)
        self._labels, self._num_groups = _vdos_labels(labels, num_groups, atoms)

    @property
    def positions_ts(self):
        return self._series.host()

    @property
    def timestep(self) -> float:
        return self._timestep

    @property
    def num_groups(self) -> int:
        return self._num_groups

    def _reducer_call(self, positions, lattices, width, starts, tau, average, device: int, **keywords):
        """The device reduction of ``positions`` and ``lattices`` (host arrays, or CUDA tensors with ``stream=``): what
        a subclass with another reducer replaces."""
        return _vdos_on_device(positions, lattices, self._masses, self._labels, self._num_groups, self._timestep, width,
                               starts, tau, average, device, **keywords)

    def _host_call(self, width, starts, tau, average):
        """The same reduction on the host."""
        return _vdos_host(self.positions_ts, self._lattices, self._masses, self._labels, self._num_groups,
                          self._timestep, width, starts, tau, average)

    def _reduce(self, table, average, device):
        width, tau, starts = table
        if device is None:
            return self._host_call(width, starts, tau, bool(average))
        positions, stream = self._series.source(int(device))
        lattices = self._lattices
        if stream is not None:
            if self._lattice_tensor is None:
                import torch
                self._lattice_tensor = torch.tensor(self._lattices, dtype=torch.float64, device=positions.device)
            lattices = self._lattice_tensor
        return self._reducer_call(positions, lattices, width, starts, tau, bool(average), int(device), stream=stream)

    def segment_starts(self, segment_steps, hop=None):
        """The first frame of each of the ``Q = (S - segment_steps) // hop + 1`` segments of ``measure_segments``; for
        an ensemble, ``(run_index, start_within_run)`` of each row of ``measure_segments(..., average=False)``."""
        return self._series.segment_starts(segment_steps, hop)

    def measure(self, device=None):
        """``(wavenumbers, D[G, bins])`` of the whole run: the one boxcar segment of all ``S`` frames.  An ensemble: the
        mean of the runs' ``VibrationalDensityOfStates.measure()``, one boxcar segment per run; a ``ValueError`` unless
        the runs have one length (their wavenumbers differ otherwise)."""
        return self._reduce(self._series.whole_table(), True, device)

    def measure_segments(self, segment_steps, hop=None, taper="hann", average=True, device=None):
        """Segment-averaged (Welch) or time-resolved VDOS on ``MDRamanSpectrum.measure_segments``' segments and axis:
        ``(wavenumbers, D[G, bins])``, the mean over the segments (taken on the power spectra), or with
        ``average=False`` the rows ``(wavenumbers, D[Q, G, bins])``.  Arguments as ``spectrum.segment_plan``."""
        return self._reduce(self._series.segment_table(segment_steps, hop, taper), average, device)


class _StepsOnDevice:
    """Mixin for a VDOS whose positions (and lattices, if per frame) stay in HBM as contiguous float64 CUDA tensors, as
    ``_OnDevice`` is for the Raman classes: the measurements reduce on the tensors' GPU unless ``host=True``; another
    ``device`` gets the host copy, which is made on first use."""

    def measure(self, device=None, host=False):
        """As the base class's ``measure``; reduces on the tensors' GPU unless ``host=True``."""
        return super().measure(device=self._series.device_or_host(device, host))

    def measure_segments(self, segment_steps, hop=None, taper="hann", average=True, device=None, host=False):
        """As the base class's ``measure_segments``; reduces on the tensors' GPU unless ``host=True``."""
        return super().measure_segments(segment_steps, hop, taper, average,
                                        device=self._series.device_or_host(device, host))


class DeviceVibrationalDensityOfStates(_StepsOnDevice, VibrationalDensityOfStates):
    """``VibrationalDensityOfStates`` of positions that already sit in HBM for the polarizability evaluation: a
    contiguous float64 CUDA tensor ``(S,N,3)``, and ``lattice`` as an array or a CUDA tensor ``(3,3)`` / ``(S,3,3)``.
    The measurements reduce on that GPU (``rn_md_vdos_device``, ordered after torch's current stream) and only the
    densities travel to the host; ``positions_ts`` copies the positions to the host on first use."""

    def __init__(self, positions_ts_device, timestep: float, lattice, masses=None, labels=None, num_groups=1):
        super().__init__(_Series.of_tensor("positions_ts", positions_ts_device, (None, None, 3)), timestep, lattice,
                         masses, labels, num_groups)


def _joined_lattices(lattice, run_lengths):
    """The lattice argument of an ensemble: one ``(3,3)`` for all runs, or a sequence of per-run ``(S_r,3,3)``, joined
    as the frames are."""
    array = np.asarray(lattice) if not isinstance(lattice, (list, tuple)) else None
    if array is not None and array.shape == (3, 3):
        return array
    parts = [np.asarray(part, dtype=np.float64) for part in lattice]
    if len(parts) != len(run_lengths) or any(part.shape != (length, 3, 3) for part, length in zip(parts, run_lengths)):
        raise ValueError("lattice must be (3,3) or one (S_r,3,3) array per run")
    return np.concatenate(parts, axis=0)


class VibrationalDensityOfStatesEnsemble(VibrationalDensityOfStates):
    """The VDOS averaged over several independent runs of one system: ``runs`` is a sequence of fractional positions
    ``(S_r,N,3)`` sharing ``timestep``, masses and labels; ``lattice`` is one ``(3,3)`` or a sequence of per-run
    ``(S_r,3,3)``.  The runs are joined end to end; the joined frames contain one step across each run boundary, which
    is computed and never read: ``measure_segments`` takes the segments of every run (``ensemble_segment_starts``; rows
    in run order, ``average=True`` the mean over all of them), ``measure`` the mean of the runs' whole VDOS, defined when
    the runs have one length."""

    def __init__(self, runs, timestep: float, lattice, masses=None, labels=None, num_groups=1):
        if not isinstance(runs, _Series):
            runs = _Series.of_runs(runs, (3,), True)
            lattice = _joined_lattices(lattice, runs.run_lengths)
        super().__init__(runs, timestep, lattice, masses, labels, num_groups)

    @property
    def run_lengths(self) -> list[int]:
        return list(self._series.run_lengths)


class DeviceVibrationalDensityOfStatesEnsemble(_StepsOnDevice, VibrationalDensityOfStatesEnsemble):
    """``VibrationalDensityOfStatesEnsemble`` whose runs stay in HBM: a sequence of contiguous float64 CUDA tensors
    ``(S_r,N,3)`` (joined here, on the GPU), or one tensor holding them end to end plus ``run_lengths``.  ``lattice``:
    ``(3,3)``, or the joined ``(sum S_r,3,3)`` as an array or a CUDA tensor."""

    def __init__(self, runs, timestep: float, lattice, masses=None, labels=None, num_groups=1, run_lengths=None):
        super().__init__(_Series.of_tensor_runs("positions_ts", runs, run_lengths, (None, None, 3)), timestep, lattice,
                         masses, labels, num_groups)


# ----------------------------------------------------------------------------- mode-projected VDOS
def mode_vectors(displacements, lattice, masses) -> NDArray[np.float64]:
    """The projection vectors of ``ModeVibrationalDensityOfStates`` from the fractional displacements ``(M,N,3)`` of
    ``Phonons``: taken to Cartesian coordinates with ``lattice`` ``(3,3)`` (rows = lattice vectors), multiplied by
    ``sqrt(masses[i])`` and normalised to unit norm over ``(N,3)`` per mode: the mass-weighted eigenvectors, orthonormal
    for a complete harmonic calculation.  ``ValueError`` for a bad shape, a non-finite entry or a mode of zero norm."""
    displacements = np.asarray(displacements)
    if displacements.ndim != 3 or displacements.shape[2] != 3 or displacements.dtype.kind not in "iuf":
        raise ValueError(f"displacements has wrong shape or type: {shape_string(displacements.shape)} != (_,_,3) reals")
    atoms = displacements.shape[1]
    lattice = np.asarray(lattice)
    if lattice.shape != (3, 3):
        raise ValueError(f"lattice has wrong shape: {shape_string(lattice.shape)} != (3,3)")
    lattice = _vdos_lattices(lattice, 1)[0]
    masses = _vdos_masses(masses, atoms)
    displacements = np.asarray(displacements, dtype=np.float64)
    if not np.all(np.isfinite(displacements)):
        raise ValueError("displacements has a non-finite entry")
    vectors = (displacements @ lattice) * np.sqrt(masses)[None, :, None]
    norms = np.sqrt((vectors ** 2).sum(axis=(1, 2)))
    if not np.all(norms > 0):
        raise ValueError(f"mode {int(np.flatnonzero(~(norms > 0))[0])} has zero norm")
    return np.ascontiguousarray(vectors / norms[:, None, None])


def _mode_vdos_vectors(vectors, atoms: int) -> NDArray[np.float64]:
    """``vectors`` ``(M,atoms,3)``, finite, ``1 <= M <= 3 atoms``, as contiguous float64."""
    if vectors is None or isinstance(vectors, (str, bytes)):
        raise get_type_error("vectors", vectors, "ndarray")
    array = np.asarray(vectors)
    if array.dtype.kind not in "iuf":
        raise get_type_error("vectors", vectors, "ndarray of real numbers")
    if array.ndim != 3 or array.shape[1:] != (atoms, 3):
        raise ValueError(f"vectors has wrong shape: {shape_string(array.shape)} != (_,{atoms},3)")
    if not 1 <= array.shape[0] <= 3 * atoms:
        raise ValueError(f"invalid number of vectors: {array.shape[0]} is not in [1, {3 * atoms}]")
    array = np.ascontiguousarray(array, dtype=np.float64)
    if not np.all(np.isfinite(array)):
        raise ValueError("vectors has a non-finite entry")
    return array


def _mode_vdos_host(positions, lattices, masses, vectors, timestep: float, width: int, starts, tau, average: bool):
    """(wavenumbers, ``D[M][bins]`` or ``D[Q][M][bins]``) on the host, from the definition (``include/rn_potgnn.h``,
    ``rn_md_mode_vdos``): per segment the tapered projections of the mass-weighted minimum-image steps onto the vectors,
    their zero-padded transforms, the power of each, its inverse transform, the positive lags and their length-n
    transform; the mean over the segments is taken on the powers.  Only the steps of the segments are read."""
    u = _vdos_steps(np.asarray(positions, dtype=np.float64), lattices) * np.sqrt(masses)[None, :, None]
    u = u.reshape(u.shape[0], -1)
    weights = vectors.reshape(vectors.shape[0], -1)
    n = width - 1
    starts = np.asarray(starts, dtype=np.int64)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    modes = weights.shape[0]
    rows = None if average else np.empty((len(starts), modes, len(keep)))
    mean = np.zeros((modes, length // 2 + 1))
    chunk = max(1, _SEGMENT_CHUNK_ELEMENTS // (length // 2 + 1))
    for q, start in enumerate(starts):
        power = np.empty((modes, length // 2 + 1))
        for first in range(0, modes, chunk):
            series = (u[start:start + n] @ weights[first:first + chunk].T) * tau[:, None]
            spectra = np.fft.rfft(series, n=length, axis=0)  # (length / 2 + 1, modes of the chunk)
            power[first:first + chunk] = (spectra.real ** 2 + spectra.imag ** 2).T
        if average:
            mean += power
        else:
            rows[q] = _lag_spectrum(power, n, length, keep)
    return wavenumbers, _lag_spectrum(mean / len(starts), n, length, keep) if average else rows


def _mode_vdos_on_device(positions, lattices, masses, vectors, timestep: float, width: int, starts, tau, average: bool,
                         device: int, stream=None, workspace_limit: int = 0):
    """(wavenumbers, ``D[M][bins]`` or ``D[Q][M][bins]``) from ``rn_md_mode_vdos`` (host positions and lattices) or, with
    two torch CUDA tensors, ``rn_md_mode_vdos_device`` ordered after ``stream``."""
    vectors = np.ascontiguousarray(vectors, dtype=np.float64)
    return _step_reducer_on_device("rn_md_mode_vdos", positions, lattices, masses, vectors, int(vectors.shape[0]),
                                   timestep, width, starts, tau, average, device, stream, workspace_limit)


class _ModeProjection:
    """Mixin that replaces the group reduction of a VDOS class by the projection onto ``vectors``: the rows are modes."""

    def _set_vectors(self, vectors) -> None:
        self._vectors = _mode_vdos_vectors(vectors, self._masses.shape[0])

    @property
    def num_modes(self) -> int:
        return self._vectors.shape[0]

    @property
    def vectors(self):
        return self._vectors.copy()

    def _reducer_call(self, positions, lattices, width, starts, tau, average, device: int, **keywords):
        return _mode_vdos_on_device(positions, lattices, self._masses, self._vectors, self._timestep, width, starts, tau,
                                    average, device, **keywords)

    def _host_call(self, width, starts, tau, average):
        return _mode_vdos_host(self.positions_ts, self._lattices, self._masses, self._vectors, self._timestep, width,
                               starts, tau, average)

    def fit_peaks(self, centres, half_width, segment_steps=None, hop=None, taper="hann", average=True,
                  fit_device=None, **measure_keywords):
        """One Lorentzian per mode row (``lineshape.fit_lorentzians``): row k is fitted on the window
        ``[centres[k] - half_width, centres[k] + half_width)`` in cm^-1.  The rows are those of ``measure`` (with
        ``segment_steps=None``: a raw periodogram, whose bins scatter by their own size, so fits belong on segment
        averages) or of ``measure_segments(segment_steps, hop, taper, average)``; ``measure_keywords`` go to that call.
        ``centres`` has ``num_modes`` entries, typically ``phonons.wavenumbers[modes]``: ``result.position - centres``
        is then the anharmonic shift and ``result.lifetime_ps`` the lifetime.  The result's arrays are ``(M,)``, or
        ``(Q,M)`` with ``average=False``.  ``fit_device`` (an int) fits on that GPU, ``None`` on the host; on the
        device-resident classes ``None`` is the tensors' GPU, unless ``host=True`` is among the keywords."""
        from ramannoodle_amd.lineshape import fit_lorentzians, mode_windows
        windows = mode_windows(centres, half_width)
        if windows.shape[0] != self.num_modes:
            raise ValueError(f"centres has wrong shape: {windows.shape[0]} entries for {self.num_modes} modes")
        if segment_steps is None:
            wavenumbers, rows = self.measure(**measure_keywords)
        else:
            wavenumbers, rows = self.measure_segments(segment_steps, hop, taper, average, **measure_keywords)
        if fit_device is None and not measure_keywords.get("host", False):
            fit_device = self._series.gpu
        return fit_lorentzians(wavenumbers, rows, np.broadcast_to(windows, rows.shape[:-1] + (2,)), device=fit_device)


class ModeVibrationalDensityOfStates(_ModeProjection, VibrationalDensityOfStates):
    """Mode-projected VDOS of an MD run (an addition): the power spectrum of the run's mass-weighted steps projected
    onto given vectors, one row per vector, on the axis of ``VibrationalDensityOfStates`` and ``MDRamanSpectrum``.  With
    the harmonic eigenvectors (``mode_vectors`` of ``Phonons.displacements``) this is the normal-mode decomposition of
    MD: row k peaks at the anharmonic frequency of mode k at the run's temperature and its width is the inverse lifetime.

    ``positions_ts``, ``timestep``, ``lattice`` and ``masses`` as for ``VibrationalDensityOfStates``; ``vectors``
    ``(M,N,3)``, finite, ``1 <= M <= 3N``, applied as given: ``D[k] = calc_signal_spectrum(y_k)`` without the zero bin,
    ``y_k[t] = sum_{i,c} vectors[k,i,c] sqrt(m_i) u[t,i,c]`` with the VDOS's step ``u``.  Scaling a vector by c scales
    its row by c^2; the rows of a complete orthonormal set sum to the one-group VDOS.  ``measure`` returns
    ``(wavenumbers, D[M, bins])``, ``measure_segments`` that or ``D[Q, M, bins]``.  ``device`` (an int) reduces on that
    GPU (``rn_md_mode_vdos``); ``None`` is the host path."""

    def __init__(self, positions_ts, timestep: float, lattice, vectors, masses=None):
        super().__init__(positions_ts, timestep, lattice, masses)
        self._set_vectors(vectors)


class DeviceModeVibrationalDensityOfStates(_StepsOnDevice, _ModeProjection, VibrationalDensityOfStates):
    """``ModeVibrationalDensityOfStates`` of positions that already sit in HBM (``DeviceVibrationalDensityOfStates``'
    arguments): reduces on that GPU (``rn_md_mode_vdos_device``, ordered after torch's current stream) unless
    ``host=True``; the mode series never leave the device."""

    def __init__(self, positions_ts_device, timestep: float, lattice, vectors, masses=None):
        super().__init__(_Series.of_tensor("positions_ts", positions_ts_device, (None, None, 3)), timestep, lattice,
                         masses)
        self._set_vectors(vectors)


class ModeVibrationalDensityOfStatesEnsemble(_ModeProjection, VibrationalDensityOfStatesEnsemble):
    """The mode-projected VDOS averaged over several independent runs of one system: ``runs`` and ``lattice`` as for
    ``VibrationalDensityOfStatesEnsemble``, ``vectors`` as for ``ModeVibrationalDensityOfStates``.  ``measure_segments``
    takes the segments of every run, ``measure`` is the mean of the runs' whole spectra (runs of one length)."""

    def __init__(self, runs, timestep: float, lattice, vectors, masses=None):
        super().__init__(runs, timestep, lattice, masses)
        self._set_vectors(vectors)


class DeviceModeVibrationalDensityOfStatesEnsemble(_StepsOnDevice, _ModeProjection,
                                                   VibrationalDensityOfStatesEnsemble):
    """``ModeVibrationalDensityOfStatesEnsemble`` whose runs stay in HBM (``DeviceVibrationalDensityOfStatesEnsemble``'s
    arguments)."""

    def __init__(self, runs, timestep: float, lattice, vectors, masses=None, run_lengths=None):
        super().__init__(_Series.of_tensor_runs("positions_ts", runs, run_lengths, (None, None, 3)), timestep, lattice,
                         masses)
        self._set_vectors(vectors)


# ----------------------------------------------------------------------------- mode-projected MD Raman spectra
def _projectors_of_vectors(vectors, lattice, masses) -> tuple[NDArray[np.float64], NDArray[np.float64]]:
    """``(D, P)`` of ``mode_projectors`` from the mass-weighted unit vectors ``e`` ``(M,N,3)`` of ``mode_vectors``."""
    root = np.sqrt(masses)[None, :, None]
    displacements = (vectors / root) @ np.linalg.inv(lattice)
    projectors = root * (vectors @ lattice.T)
    return np.ascontiguousarray(displacements), np.ascontiguousarray(projectors)


def mode_projectors(displacements, lattice, masses) -> tuple[NDArray[np.float64], NDArray[np.float64]]:
    """The two sets of vectors of ``ModeMDRamanSpectrum`` from the fractional displacements ``(M,N,3)`` of ``Phonons``,
    a pair of float64 arrays ``(D, P)``, each ``(M,N,3)``.  With ``e = mode_vectors(displacements, lattice, masses)``,
    the mass-weighted unit eigenvectors: ``D[m,i] = (e[m,i] / sqrt(masses[i])) @ inv(lattice)``, the fractional
    displacement of a unit amplitude of mode m, and ``P[m,i] = sqrt(masses[i]) * (e[m,i] @ lattice.T)``, the mode's dual
    in fractional coordinates: ``P[m] . dx`` is the amplitude of mode m in a fractional step ``dx``.  For a complete
    orthonormal ``e``, ``sum_m D[m,i,a] P[m,j,b] = delta_ij delta_ab``.  ``ValueError`` as ``mode_vectors``."""
    vectors = mode_vectors(displacements, lattice, masses)
    return _projectors_of_vectors(vectors, _vdos_lattices(lattice, 1)[0], _vdos_masses(masses, vectors.shape[1]))


def _md_modes_host(increments, timestep: float, weights, width: int, starts, tau, average: bool):
    """(wavenumbers, ``I[K,C+1,bins]`` or ``I[Q,K,C+1,bins]``) on the host, from the definition (``include/rn_potgnn.h``,
    ``rn_md_raman_modes``): channel ``C`` is the sum of the ``C`` channels; per segment of ``width`` frames starting at
    frame ``starts[q]`` the zero-padded transforms of the tapered components of increments ``starts[q] .. starts[q] +
    width - 2`` of each channel, their power contracted with each configuration's form, its inverse transform, the
    positive lags and their length-n transform; the mean over the segments is taken on the contracted powers."""
    d = _symmetric_components(np.asarray(increments, dtype=np.float64))  # (N, C, 6)
    d = np.concatenate([d, d.sum(axis=1, keepdims=True)], axis=1)
    channels = d.shape[1]
    n = width - 1
    starts = np.asarray(starts, dtype=np.int64)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    forms = _weight_forms(weights)
    count = weights.shape[0]
    out = None if average else np.empty((len(starts), count, channels, len(keep)))
    mean = np.zeros((count, channels, length // 2 + 1))
    chunk = max(1, _SEGMENT_CHUNK_ELEMENTS // ((length // 2 + 1) * 6))  # channels of one segment at once
    for q, start in enumerate(starts):
        for first in range(0, channels, chunk):
            series = d[start:start + n, first:first + chunk] * tau[:, None, None]
            spectra = np.fft.rfft(series, n=length, axis=0)  # (length / 2 + 1, c, 6)
            power = np.einsum("kje,fcj,fce->kcf", forms, spectra, np.conj(spectra)).real
            if average:
                mean[:, first:first + chunk] += power
            else:
                out[q, :, first:first + chunk] = _lag_spectrum(power, n, length, keep)
    if average:
        out = _lag_spectrum(mean / len(starts), n, length, keep)
    return wavenumbers, out


def _md_modes_on_device(increments, timestep: float, weights, width: int, starts, tau, average: bool, device: int,
                        stream=None, workspace_limit: int = 0):
    """(wavenumbers, uncorrected ``I[K,C+1,bins]`` or ``I[Q,K,C+1,bins]``) from ``rn_md_raman_modes`` (host increments)
    or, with a torch CUDA tensor, ``rn_md_raman_modes_device`` ordered after ``stream``."""
    import ctypes as C
    steps, channels = increments.shape[0], increments.shape[1]
    weights, weight_args = _weights_arguments(weights)
    starts, table_args = _table_arguments(starts)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    count = weights.shape[0]
    shape = (count, channels + 1) if average else (len(starts), count, channels + 1)
    return _call_md_reducer(
        "rn_md_raman_modes", increments, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
        (steps, channels, width, *table_args, C.c_void_p(tau.ctypes.data), *weight_args, int(bool(average))),
        (workspace_limit,))


def band_weights(wavenumbers, bands, laser_correction=False, laser_wavelength=522, bose_einstein_correction=False,
                 temperature=300) -> NDArray[np.float64]:
    """The weights ``bw[B,bins]`` that sum a spectrum on ``wavenumbers`` ``(bins,)`` over ``bands`` ``(B,2)``, the
    half-open intervals ``[lo, hi)`` in cm^-1: 1 for a bin inside its band, 0 outside, times the laser and
    Bose-Einstein corrections of the bin where asked for, so that ``bw @ I`` is the band sums of the corrected rows
    ``I[..., bins]``.  ``ValueError``: ``bands`` of another shape or with no band, a non-finite edge, ``lo >= hi``, and
    a band that holds no bin (the message names the band and the bin spacing).  What ``measure_interference`` hands to
    ``rn_md_raman_mode_matrix``."""
    wavenumbers = np.asarray(wavenumbers, dtype=np.float64)
    try:
        edges = np.asarray(bands, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError("bands must be an array (B,2) of band edges in cm^-1") from exc
    if edges.ndim != 2 or edges.shape[1] != 2 or edges.shape[0] < 1:
        raise ValueError(f"bands has wrong shape: {shape_string(edges.shape)} != (_,2)")
    if not np.all(np.isfinite(edges)):
        raise ValueError("bands has a non-finite edge")
    for index, (low, high) in enumerate(edges):
        if low >= high:
            raise ValueError(f"bands[{index}] is empty: {low:g} >= {high:g}")
    inside = (wavenumbers[None, :] >= edges[:, :1]) & (wavenumbers[None, :] < edges[:, 1:])
    for index in np.flatnonzero(~inside.any(axis=1)):
        spacing = wavenumbers[0]  # (the bins are the multiples of the first)
        raise ValueError(f"bands[{index}] = [{edges[index, 0]:g}, {edges[index, 1]:g}) cm^-1 holds no bin: the bins are "
                         f"{spacing:g} cm^-1 apart, from {wavenumbers[0]:g} to {wavenumbers[-1]:g}")
    weights = _apply_corrections(wavenumbers, inside.astype(np.float64), laser_correction, laser_wavelength,
                                 bose_einstein_correction, temperature)
    return np.ascontiguousarray(weights, dtype=np.float64)


def _md_mode_matrix_host(increments, timestep: float, weights, width: int, starts, tau, bin_weights):
    """``A[B,K,C,C]`` on the host, from the definition (``include/rn_potgnn.h``, ``rn_md_raman_mode_matrix``): per
    segment the zero-padded transforms of the tapered components of each channel, for each pair of channels their
    cross-power contracted with each configuration's form and averaged over the segments, its inverse transform, the
    positive lags and their length-n transform (the pair spectra of ``_md_partial_segments_host`` without a cap on the
    channels), and then the sum over the bins with ``bin_weights``.  Pairs ``m <= n`` are computed and mirrored."""
    d = _symmetric_components(np.asarray(increments, dtype=np.float64))  # (N, C, 6)
    channels = d.shape[1]
    n = width - 1
    starts = np.asarray(starts, dtype=np.int64)
    wavenumbers, keep, length = _lag_axis(n, timestep)
    forms = _weight_forms(weights)
    count = weights.shape[0]
    power = np.zeros((count, channels, channels, length // 2 + 1))  # rows m, columns n >= m
    for start in starts:
        spectra = np.fft.rfft(d[start:start + n] * tau[:, None, None], n=length, axis=0)  # (length / 2 + 1, C, 6)
        for m in range(channels):
            cross = np.real(spectra[:, m, None, :, None] * np.conj(spectra[:, m:, None, :]))  # (f, n, j, l)
            power[:, m, m:] += np.einsum("kje,fnje->knf", forms, cross)
    spectra_of_pairs = _lag_spectrum(power / len(starts), n, length, keep)  # (K, C, C, bins)
    out = np.einsum("bi,kmni->bkmn", np.asarray(bin_weights, dtype=np.float64), spectra_of_pairs)
    rows, cols = np.triu_indices(channels, 1)
    out[:, :, cols, rows] = out[:, :, rows, cols]
    return out


def _md_mode_matrix_on_device(increments, timestep: float, weights, width: int, starts, tau, bin_weights, device: int,
                              stream=None, workspace_limit: int = 0):
    """``A[B,K,C,C]`` from ``rn_md_raman_mode_matrix`` (host increments) or, with a torch CUDA tensor,
    ``rn_md_raman_mode_matrix_device`` ordered after ``stream``."""
    import ctypes as C
    steps, channels = increments.shape[0], increments.shape[1]
    weights, weight_args = _weights_arguments(weights)
    starts, table_args = _table_arguments(starts)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    bin_weights = np.ascontiguousarray(bin_weights, dtype=np.float64)
    if bin_weights.ndim != 2 or bin_weights.shape[1] != width // 2 - 1:
        raise ValueError(f"bin_weights has wrong shape: {shape_string(bin_weights.shape)}")
    shape = (bin_weights.shape[0], weights.shape[0], channels, channels)
    _, out = _call_md_reducer(
        "rn_md_raman_mode_matrix", increments, width - 1, _TOO_FEW_STEPS, timestep, device, stream, shape,
        (steps, channels, width, *table_args, C.c_void_p(tau.ctypes.data), *weight_args,
         C.c_void_p(bin_weights.ctypes.data), bin_weights.shape[0]), (workspace_limit,), bin_axis=False)
    return out


MAX_SELECTED = MAX_GROUPS - 1  # channels of ModeMDRamanSpectrum.select, beside the channel of all others


class ModeMDRamanSpectrum(_ContractedMDSpectrum):
    """Phonon-mode decomposition of an MD spectrum: per-channel polarizability increments ``(S-1,C,3,3)``
    (``PotGNN.calc_mode_increments``: the modes, then the rest and the cell where present) and a timestep in fs.  Every
    measurement returns ``(wavenumbers, I[..., C+1, bins])``: row ``c < C`` is the self-spectrum of channel c, what
    ``PartialMDRamanSpectrum`` calls ``I[g,g]``, and the last row the spectrum of the summed increments, the whole
    spectrum; ``I[..., C, :] - I[..., :C, :].sum(-2)`` is the interference between channels.  Any number of channels;
    which of them interfere under a peak comes from ``measure_interference``, the matrix of all pair spectra summed
    over a band, and the pair spectra of a few channels bin by bin from ``select``.  ``device`` (an int) reduces on
    that GPU (``rn_md_raman_modes``, ``rn_md_raman_mode_matrix``); arguments and corrections are those of
    ``PartialMDRamanSpectrum``.

    ``measure`` returns ``(wavenumbers, I[C+1,bins])`` of ``measure()``'s ``45 a^2 + 7 gamma^2`` over the whole run,
    ``measure_polarized`` ``(wavenumbers, I[K,C+1,bins])`` for the configurations of ``polarized_weights``;
    ``[C+1,bins]`` when no argument has a ``K`` axis.  ``measure_segments``: segment-averaged (Welch) or time-resolved
    spectra over ``PartialMDRamanSpectrum.measure_segments``' segments: ``(wavenumbers, I[C+1,bins])``, or
    ``I[Q,C+1,bins]`` with ``average=False``; ``measure_segments_polarized`` ``I[K,C+1,bins]``, or ``I[Q,K,C+1,bins]``
    with ``average=False``; the ``K`` axis is squeezed when no argument has one."""

    _row_axes = 1

    def __init__(self, increments, timestep: float):
        super().__init__(_held("increments", increments, (None, None, 3, 3), increments=True), timestep)
        if self._series.shape[1] < 1:
            raise ValueError("increments has no channel")

    @property
    def increments(self):
        return self._series.host()

    @property
    def num_channels(self) -> int:
        return self._series.shape[1]

    def _whole_table(self):
        return self._series.whole_table(_TOO_FEW_STEPS)

    def _reduce(self, weights, table, average: bool, device):
        width, tau, starts = table
        if device is None:
            return _md_modes_host(self._series.host(), self._timestep, weights, width, starts, tau, bool(average))
        source, stream = self._series.source(int(device))
        return _md_modes_on_device(source, self._timestep, weights, width, starts, tau, bool(average), int(device),
                                   stream=stream)

    def _interference(self, weights, bands, segment_steps, hop, taper, corrections, device):
        """``(bands, A[B,K,C,C])`` of both interference measurements; ``corrections``: the four correction arguments."""
        if segment_steps is None:
            width, tau, starts = self._whole_table()
        else:
            width, tau, starts = self._series.segment_table(segment_steps, hop, taper)
        n = width - 1
        wavenumbers = (scipy.fftpack.fftfreq(n, self._timestep) * _PER_FS_TO_CM1)[1:(n + 1) // 2]
        if len(wavenumbers) == 0:
            raise ValueError(f"segments of {width} frames have no bin to sum over")
        weights_of_bins = band_weights(wavenumbers, bands, *corrections)
        if device is not None:
            source, stream = self._series.source(int(device))
            matrices = _md_mode_matrix_on_device(source, self._timestep, weights, width, starts, tau, weights_of_bins,
                                                 int(device), stream=stream)
        else:
            matrices = _md_mode_matrix_host(self._series.host(), self._timestep, weights, width, starts, tau,
                                            weights_of_bins)
        return np.array(bands, dtype=np.float64), matrices

    def measure_interference(self, bands, segment_steps=None, hop=None, taper="hann", orientation="polycrystalline",
                             laser_correction=False, laser_wavelength=522, bose_einstein_correction=False,
                             temperature=300, device=None):
        """Which channels interfere under a peak: ``(bands, A[B,C,C])``, the pair spectra between all channels summed
        over each of ``bands`` ``(B,2)`` (cm^-1, half-open ``[lo, hi)``; ``band_weights``).  ``A[b,m,n]`` is the band
        sum of what ``PartialMDRamanSpectrum.measure_segments`` calls ``I[m,n]``, for any number of channels:
        symmetric, ``A[b].sum()`` the band sum of the whole spectrum (the last row of ``measure_segments``),
        ``np.diagonal(A[b])`` the band sums of the self-spectra and ``A[b].sum(-1)`` each channel's share of the band
        with its cross terms, shares that add up to the band as the self-spectra do not.  ``segment_steps``, ``hop``
        and ``taper`` as for ``measure_segments``, always the segment mean; ``segment_steps=None`` is the whole run as
        one boxcar segment, as ``measure``.  The corrections weight the bins before the sum.  ``device`` (an int)
        reduces on that GPU (``rn_md_raman_mode_matrix``: one float64 matrix product); ``None`` is the host, from the
        definition, whose time and memory grow with ``C^2``.  ``ValueError`` for ``bands``: see ``band_weights``."""
        _require_polycrystalline(orientation)
        corrections = (laser_correction, laser_wavelength, bose_einstein_correction, temperature)
        bands, matrices = self._interference(_measure_weights(), bands, segment_steps, hop, taper, corrections, device)
        return bands, matrices[:, 0]

    def measure_interference_polarized(self, incident, scattered, orientation=None, *, bands, segment_steps=None,
                                       hop=None, taper="hann", laser_correction=False, laser_wavelength=522,
                                       bose_einstein_correction=False, temperature=300, device=None):
        """``measure_interference`` for the configurations of ``polarized_weights``: ``(bands, A[K,B,C,C])``;
        ``[B,C,C]`` when no argument has a ``K`` axis."""
        weights, squeeze = polarized_weights(incident, scattered, orientation)
        corrections = (laser_correction, laser_wavelength, bose_einstein_correction, temperature)
        bands, matrices = self._interference(weights, bands, segment_steps, hop, taper, corrections, device)
        matrices = np.ascontiguousarray(np.swapaxes(matrices, 0, 1))
        return bands, matrices[0] if squeeze else matrices

    def _selection(self, channels) -> tuple[NDArray[np.int64], NDArray[np.int64]]:
        """``(channels, all others)`` of ``select``."""
        index = np.asarray(channels)
        if index.dtype.kind not in "iu" or index.ndim != 1:
            raise ValueError("channels must be a one-dimensional integer array")
        if not 1 <= index.size <= MAX_SELECTED:
            raise ValueError(f"select takes 1 to {MAX_SELECTED} channels, not {index.size}")
        if index.min() < 0 or index.max() >= self.num_channels:
            raise ValueError(f"channels must lie in [0, {self.num_channels})")
        if len(np.unique(index)) != index.size:
            raise ValueError("channels names a channel twice")
        return index.astype(np.int64), np.setdiff1d(np.arange(self.num_channels), index)

    def _selected(self, channels):
        """The increments of ``select``, where the series lives: the chosen channels, then the sum of all others."""
        index, others = self._selection(channels)
        if self._series.gpu is None:
            increments = np.asarray(self._series.host())
            chosen = np.concatenate([increments[:, index], increments[:, others].sum(axis=1, keepdims=True)], axis=1)
            return np.ascontiguousarray(chosen)
        import torch
        tensor = self._series.data
        chosen = torch.cat([tensor[:, torch.as_tensor(index, device=tensor.device)],
                            tensor[:, torch.as_tensor(others, device=tensor.device)].sum(dim=1, keepdim=True)], dim=1)
        return chosen.contiguous()

    def select(self, channels):
        """A ``PartialMDRamanSpectrum`` of the chosen ``channels`` (1 to 15 distinct indices, in the order given) plus
        one last channel holding the sum of all others: its ``I[g,h]`` are the pair spectra of the chosen modes, cross
        terms included, and its sum over all pairs is the whole spectrum."""
        return PartialMDRamanSpectrum(self._selected(channels), self._timestep)


class _InterferenceOnDevice(_OnDevice):
    """``_OnDevice`` for the mode spectra, which have the two interference measurements as well."""

    def measure_interference(self, bands, segment_steps=None, hop=None, taper="hann", orientation="polycrystalline",
                             laser_correction=False, laser_wavelength=522, bose_einstein_correction=False,
                             temperature=300, device=None, host=False):
        """As the base class's ``measure_interference``; reduces on the tensor's GPU unless ``host=True``."""
        return super().measure_interference(bands, segment_steps, hop, taper, orientation, laser_correction,
                                            laser_wavelength, bose_einstein_correction, temperature,
                                            device=self._series.device_or_host(device, host))

    def measure_interference_polarized(self, incident, scattered, orientation=None, *, bands, segment_steps=None,
                                       hop=None, taper="hann", laser_correction=False, laser_wavelength=522,
                                       bose_einstein_correction=False, temperature=300, device=None, host=False):
        """As the base class's ``measure_interference_polarized``; reduces on the tensor's GPU unless ``host=True``."""
        return super().measure_interference_polarized(
            incident, scattered, orientation, bands=bands, segment_steps=segment_steps, hop=hop, taper=taper,
            laser_correction=laser_correction, laser_wavelength=laser_wavelength,
            bose_einstein_correction=bose_einstein_correction, temperature=temperature,
            device=self._series.device_or_host(device, host))


class DeviceModeMDRamanSpectrum(_InterferenceOnDevice, ModeMDRamanSpectrum):
    """``ModeMDRamanSpectrum`` whose increments stay in HBM (a contiguous float64 CUDA tensor ``(S-1,C,3,3)``): the
    measurements reduce them on that GPU (``rn_md_raman_modes_device``, ``rn_md_raman_mode_matrix_device``, ordered
    after torch's current stream) unless ``host=True``; ``increments`` copies them to the host on first use.
    ``select`` returns a ``DevicePartialMDRamanSpectrum``."""

    def __init__(self, increments_device, timestep: float):
        super().__init__(_Series.of_tensor("increments", increments_device, (None, None, 3, 3), increments=True),
                         timestep)

    def select(self, channels):
        return DevicePartialMDRamanSpectrum(self._selected(channels), self._timestep)


class ModeMDRamanEnsemble(_Ensemble, ModeMDRamanSpectrum):
    """Phonon-mode spectra averaged over several runs: ``runs`` is a sequence of per-channel increments
    ``(S_r-1,C,3,3)`` sharing ``C`` and ``timestep``.  The runs are joined with one zero row between them, so that
    increment t still belongs to frame t of the joined frames; no segment reads that row.  Every measurement of
    ``ModeMDRamanSpectrum`` is here: the segment measurements and ``measure_interference`` with ``segment_steps`` take
    the segments of every run (``ensemble_segment_starts`` of the runs' ``S_r`` frames; rows in run order,
    ``average=True`` the mean over all of them); ``measure`` / ``measure_polarized`` and ``measure_interference``
    without ``segment_steps`` the mean over the runs of each run's whole spectrum, one boxcar segment per run, when
    the runs have one length.  ``device`` (an int) reduces all runs in one call.  ``select`` returns a
    ``PartialMDRamanEnsemble``."""

    def __init__(self, runs, timestep: float):
        super().__init__(runs if isinstance(runs, _Series) else _Series.of_runs(runs, (3, 3), True, increments=True),
                         timestep)

    def select(self, channels):
        chosen = self._selected(channels)
        lengths = self._series.run_lengths
        return PartialMDRamanEnsemble([chosen[end - length:end - 1] for length, end in zip(lengths, np.cumsum(lengths))],
                                      self._timestep)


class DeviceModeMDRamanEnsemble(_InterferenceOnDevice, ModeMDRamanEnsemble):
    """``ModeMDRamanEnsemble`` whose increments stay in HBM: a sequence of contiguous float64 CUDA tensors
    ``(S_r-1,C,3,3)`` (joined here, on the GPU, with a zero row between them), or one tensor ``(sum(S_r)-1,C,3,3)``
    plus ``run_lengths`` (frames per run), as one batched evaluation of the joined frames writes it: its rows across
    the run boundaries stand where the zero rows would and are never read.  ``select`` returns a
    ``DevicePartialMDRamanEnsemble``."""

    def __init__(self, runs, timestep: float, run_lengths=None):
        super().__init__(_Series.of_tensor_runs("runs", runs, run_lengths, (None, None, 3, 3), increments=True,
                                                tensors_only=True), timestep)

    def select(self, channels):
        return DevicePartialMDRamanEnsemble(self._selected(channels), self._timestep, self._series.run_lengths)

