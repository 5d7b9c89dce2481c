"""What the device models (``PotGNN``, ``InterpolationModel``) share on the host side of their device entries: the checks
of positions, result tensors, mode vectors and Raman arguments, and ``DeviceIncrements``, the part of the contract
``ramannoodle_amd.dynamics`` looks for that is the same for every model."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ramannoodle_amd import _lib
from ramannoodle_amd.exceptions import verify_ndarray_shape


def _ptr(array) -> C.c_void_p:
    return C.c_void_p(array.ctypes.data)


def device_frames(positions, num_atoms: int, least: int, what: str, device_index=None) -> int:
    """The frame count of the device positions of an entry after their checks: a contiguous CUDA float64 ``(S,N,3)``
    tensor of at least ``least`` frames, on ``cuda:device_index`` unless that is ``None``."""
    if not (isinstance(positions, torch.Tensor) and positions.is_cuda and positions.dtype == torch.float64
            and positions.is_contiguous()):
        raise ValueError("positions must be a contiguous float64 device tensor")
    if device_index is not None and positions.device.index != device_index:
        raise ValueError(f"positions live on {positions.device}, the model on cuda:{device_index}")
    if positions.dim() != 3 or tuple(positions.shape[1:]) != (num_atoms, 3):
        raise ValueError(f"positions has wrong shape: {tuple(positions.shape)} != (_,{num_atoms},3)")
    if positions.shape[0] < least:
        raise ValueError(f"{what} needs at least {least} frame(s), not {positions.shape[0]}")
    return positions.shape[0]


def _checked_out(out, device_index: int, shape, written_on: str, written_as: str):
    """A caller's result tensor, through whose pointer the library writes ``prod(shape)`` float64 values: checked before
    anything reaches the library (a leading slice ``out[:s]`` of a larger tensor is contiguous and passes)."""
    if not isinstance(out, torch.Tensor):
        raise ValueError(f"out must be a torch.Tensor, not {type(out).__name__}")
    if not out.is_cuda or out.device.index != device_index:
        raise ValueError(f"out lives on {out.device}, {written_on}")
    if out.dtype != torch.float64:
        raise ValueError(f"out must be float64, not {out.dtype}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"out has shape {tuple(out.shape)}, {written_as}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    return out


def device_out(out, positions, shape, what: str = "the result"):
    """``out`` of a device entry after its checks, or a new float64 tensor of ``shape`` on the positions' device."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=positions.device)
    return _checked_out(out, positions.device.index, shape, f"{what} is written on {positions.device}",
                        f"{what} is {tuple(shape)}")


def check_out(out, s: int, device_index: int) -> None:
    """``device_out`` for the ``(s,3,3)`` result of an evaluation that is given a device index, not positions."""
    _checked_out(out, device_index, (s, 3, 3), f"the evaluation writes on cuda:{device_index}",
                 f"the evaluation writes ({s}, 3, 3)")


def mode_arrays(displacements, projectors, num_atoms: int):
    """``displacements`` and ``projectors`` ``(M,N,3)``, finite, as contiguous float64 (``spectrum.mode_projectors``)."""
    arrays = []
    for name, value in (("displacements", displacements), ("projectors", projectors)):
        if value is None or isinstance(value, (str, bytes, torch.Tensor)):
            raise ValueError(f"{name} must be a host array (M,{num_atoms},3)")
        array = np.asarray(value)
        if array.dtype.kind not in "iuf":
            raise ValueError(f"{name} must hold real numbers, not {array.dtype}")
        if array.ndim != 3 or array.shape[0] < 1 or tuple(array.shape[1:]) != (num_atoms, 3):
            raise ValueError(f"{name} has wrong shape: {tuple(array.shape)} != (_,{num_atoms},3)")
        array = np.ascontiguousarray(array, dtype=np.float64)
        if not np.all(np.isfinite(array)):
            raise ValueError(f"{name} has a non-finite entry")
        arrays.append(array)
    if arrays[0].shape != arrays[1].shape:
        raise ValueError(f"displacements {arrays[0].shape} and projectors {arrays[1].shape} differ in shape")
    return arrays


def raman_arguments(ref_positions, displacements, delta, method, num_atoms: int) -> None:
    """The argument checks of ``calc_raman_tensors``."""
    verify_ndarray_shape("ref_positions", ref_positions, (num_atoms, 3))
    verify_ndarray_shape("displacements", displacements, (None, num_atoms, 3))
    if method not in ("finite-difference", "analytic"):
        raise ValueError(f"unsupported method: {method}")
    if method == "finite-difference" and not (np.isfinite(delta) and float(delta) != 0.0):
        raise ValueError(f"delta must be finite and non-zero, not {delta}")


def host_positions_to_device(name: str, positions_ts, num_atoms: int, device_index: int, lattices=None):
    """Host positions ``(S,N,3)`` and lattices (``(S,3,3)``, or ``None``) after their checks -- non-finite or singular
    lattices raise ``ValueError`` -- as float64 tensors on ``cuda:device_index``."""
    verify_ndarray_shape(name, positions_ts, (None, num_atoms, 3))
    if lattices is not None:
        from ramannoodle_amd.dynamics import verify_lattices
        lattices = verify_lattices(lattices, len(positions_ts))
    device = f"cuda:{device_index}"
    positions = torch.tensor(np.asarray(positions_ts, dtype=np.float64), device=device)
    return positions, None if lattices is None else torch.tensor(lattices, device=device)


class DeviceIncrements:
    """The entries of a device model that are written once.  A model brings ``num_atoms``, ``device_index``,
    ``_ref_structure``, ``_ensure_handle``, its ``calc_*_increments_device``, and the two names below."""

    _partial_raman_entry: str  # the library's partial_raman_tensors entry of the model
    _check_status = None       # its status check, a staticmethod: _lib.check or _lib.check_interp

    def _group_labels(self, groups):
        from ramannoodle_amd.spectrum import group_labels
        return group_labels(groups, self._ref_structure.atomic_numbers)

    def _increments_from_host(self, entry, positions_ts, lattices, *args, **kwargs):
        """``entry``, one of the model's ``calc_*_increments_device``, for host positions and lattices."""
        positions, lattices = host_positions_to_device("positions_ts", positions_ts, self.num_atoms, self.device_index,
                                                       lattices)
        return entry(positions, *args, lattices=lattices, **kwargs).cpu().numpy()

    def _partial_raman_tensors(self, ref_positions, displacements, groups):
        """``(M,G,3,3)`` from the model's partial_raman_tensors entry; the arguments are already checked."""
        labels, num_groups = self._group_labels(groups)
        ref = np.ascontiguousarray(ref_positions, dtype=np.float64)
        disp = np.ascontiguousarray(displacements, dtype=np.float64)
        out = np.empty((disp.shape[0], num_groups, 3, 3), dtype=np.float64)
        handle = self._ensure_handle()
        rc = getattr(_lib.load(), self._partial_raman_entry)(handle, _ptr(ref), _ptr(disp), disp.shape[0], _ptr(labels),
                                                             num_groups, _ptr(out))
        self._check_status(rc, handle, self._partial_raman_entry)
        return out
