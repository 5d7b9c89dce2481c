"""Interpolation polarizability model (``ramannoodle/pmodel/_interpolation.py``, ``_art.py``) evaluated on the GPU.

The model is data: a reference structure and polarizability, ``J`` Cartesian basis vectors (degrees of freedom) and one
spline with 3x3 values per degree of freedom.  Building one (symmetry expansion, ``add_dof``, file readers) is the
reference's job; this class takes a finished model (``InterpolationModel.from_reference``) and offers every method
``ramannoodle_amd.dynamics`` looks for, so that it yields the spectra a ``PotGNN`` yields for a fixed cell.

Definition, all float64 (``include/rn_interp.h`` has the device's statement of it):

* wrapped displacement ``d = x - x_ref``, ``m = d - floor(d)``, ``w = m - 1 if m > 0.5 else m`` (the reference's
  ``apply_pbc_displacement``: exactly +0.5 stays +0.5 and -0.5 becomes +0.5; it is not ``d - rint(d)``);
* amplitude ``a_j = sum_{i,r} w[i][r] F[j][3i+r]`` with ``F[j][3i+r] = sum_s L[r][s] b_j[i][s]``;
* per-piece Taylor tables of every spline (``piecewise_tables``); the value at ``a`` is Horner in ``u = a - x_p`` on
  piece ``p``, the end pieces extending beyond the knots (scipy's ``extrapolate=True``);
* ``alpha(x) = alpha_ref + sum_j (1 - mask_j) s_j(a_j)``;
* Jacobian ``d alpha / d x_{i,r} = sum_j (1 - mask_j) s_j'(a_j) F[j][3i+r]``, rows ``[frame][6][N][3]`` in the
  component order ``(xx, yy, zz, xy, xz, yz)``.

``piecewise_tables`` and ``evaluate_host`` carry this definition in numpy; the device is tested against them.  The
evaluation itself has no CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import NamedTuple

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd import _lib
from ramannoodle_amd.abstract import PolarizabilityModel
from ramannoodle_amd.constants import RAMAN_TENSOR_CENTRAL_DIFFERENCE
from ramannoodle_amd.exceptions import verify_ndarray_shape
from ramannoodle_amd.pmodel._device import (DeviceIncrements, _ptr, device_frames, device_out, mode_arrays,
                                            raman_arguments)

MAX_ORDER = 5  # RN_INTERP_MAX_ORDER of include/rn_interp.h
SYMMETRY_TOLERANCE = 1e-12  # asymmetry of the tables, relative to the largest coefficient
_VEC6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


class PiecewiseTables(NamedTuple):
    """The splines of a model as per-piece Taylor tables (the arguments of ``rn_interp_create``): DOF ``j`` has
    ``piece_offsets[j+1] - piece_offsets[j]`` pieces, its breakpoints ``x_0 < .. < x_P`` start at
    ``breakpoints[piece_offsets[j] + j]``, and the coefficients ``c[p][q] = s^(q)(x_p) / q!`` (``q = 0..orders[j]``,
    nine components each) of its pieces follow each other in ``coefficients``, DOF after DOF."""

    piece_offsets: NDArray[np.int32]
    breakpoints: NDArray[np.float64]
    orders: NDArray[np.int32]
    coefficients: NDArray[np.float64]


def piecewise_tables(interpolations) -> PiecewiseTables:
    """The tables of ``interpolations``, a sequence of ``scipy.interpolate.BSpline`` with values of shape ``(3,3)``.
    The breakpoints of DOF ``j`` of order ``k`` are the unique knots of the base interval ``t[k] .. t[len(t)-k-1]`` and
    the coefficients come from the spline itself (``spline(x, nu=q)``, right-continuous).  ``ValueError``: no spline at
    all (a dummy model), an order outside 1..5 (the message names the DOF), values that are not ``(3,3)``, or a
    non-finite table."""
    interpolations = list(interpolations)
    if not interpolations:
        raise ValueError("the model has no interpolations (a dummy model cannot calculate polarizabilities)")
    offsets, breakpoints, orders, coefficients = [0], [], [], []
    for j, spline in enumerate(interpolations):
        try:
            knots, order = np.asarray(spline.t, dtype=np.float64), int(spline.k)
            shape = tuple(np.shape(spline.c)[1:])
        except AttributeError as exc:
            raise ValueError(f"interpolations[{j}] is not a BSpline") from exc
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"interpolations[{j}] has order {order}: orders 1..{MAX_ORDER} are supported")
        if shape != (3, 3):
            raise ValueError(f"interpolations[{j}] has values of shape {shape}, not (3, 3)")
        xs = np.unique(knots[order:len(knots) - order])
        if len(xs) < 2 or not np.all(np.isfinite(xs)):
            raise ValueError(f"interpolations[{j}] has no finite base interval")
        table = np.empty((len(xs) - 1, order + 1, 9))
        factorial = 1.0
        for q in range(order + 1):
            factorial *= max(q, 1)
            table[:, q] = np.asarray(spline(xs[:-1], nu=q), dtype=np.float64).reshape(-1, 9) / factorial
        if not np.all(np.isfinite(table)):
            raise ValueError(f"interpolations[{j}] has a non-finite table")
        offsets.append(offsets[-1] + len(xs) - 1)
        breakpoints.append(xs)
        orders.append(order)
        coefficients.append(table.reshape(-1))
    return PiecewiseTables(np.array(offsets, dtype=np.int32), np.concatenate(breakpoints),
                           np.array(orders, dtype=np.int32), np.concatenate(coefficients))


def wrapped_displacement(positions, ref_positions) -> NDArray[np.float64]:
    """``w`` of the module's definition for fractional ``positions`` ``(...,N,3)`` about ``ref_positions`` ``(N,3)``."""
    d = np.asarray(positions, dtype=np.float64) - np.asarray(ref_positions, dtype=np.float64)
    m = d - np.floor(d)
    return np.where(m > 0.5, m - 1.0, m)


def folded_basis(lattice, cart_basis_vectors) -> NDArray[np.float64]:
    """``F`` ``(J,3N)``: the Cartesian basis vectors ``(J,N,3)`` with the lattice (rows = vectors) folded in."""
    basis = np.asarray(cart_basis_vectors, dtype=np.float64)
    return np.einsum("rs,jis->jir", np.asarray(lattice, dtype=np.float64), basis).reshape(len(basis), -1)


def amplitudes_host(lattice, ref_positions, cart_basis_vectors, positions) -> NDArray[np.float64]:
    """The amplitudes ``(S,J)`` of ``positions`` ``(S,N,3)``."""
    w = wrapped_displacement(positions, ref_positions)
    return w.reshape(len(w), -1) @ folded_basis(lattice, cart_basis_vectors).T


def evaluate_host(tables: PiecewiseTables, lattice, ref_positions, ref_polarizability, cart_basis_vectors, positions,
                  mask=None, jacobian: bool = False):
    """The model's definition in numpy: polarizabilities ``(S,3,3)`` of the fractional ``positions`` ``(S,N,3)`` and,
    with ``jacobian=True``, also the Jacobian rows ``(S,6,N,3)`` (the six components read off the upper triangle)."""
    positions = np.asarray(positions, dtype=np.float64)
    frames, atoms = positions.shape[0], positions.shape[1]
    folded = folded_basis(lattice, cart_basis_vectors)
    w = wrapped_displacement(positions, ref_positions)
    amplitudes = w.reshape(frames, -1) @ folded.T
    dofs = len(tables.orders)
    scale = np.ones(dofs) if mask is None else 1.0 - np.asarray(mask, dtype=np.float64)
    delta = np.zeros((frames, 9))
    slopes = np.zeros((frames, dofs, 9)) if jacobian else None
    start = 0
    for j in range(dofs):
        first, pieces, order = int(tables.piece_offsets[j]), int(tables.piece_offsets[j + 1] - tables.piece_offsets[j]), \
            int(tables.orders[j])
        xs = tables.breakpoints[first + j:first + j + pieces + 1]
        table = tables.coefficients[start:start + pieces * (order + 1) * 9].reshape(pieces, order + 1, 9)
        start += pieces * (order + 1) * 9
        a = amplitudes[:, j]
        piece = np.clip(np.searchsorted(xs, a, side="right") - 1, 0, pieces - 1)
        u = (a - xs[piece])[:, None]
        c = table[piece]  # (S, order+1, 9)
        value = c[:, order]
        for q in range(order - 1, -1, -1):
            value = value * u + c[:, q]
        delta += scale[j] * value
        if jacobian:
            slope = order * c[:, order]
            for q in range(order - 1, 0, -1):
                slope = slope * u + q * c[:, q]
            slopes[:, j] = scale[j] * slope
    alpha = (delta + np.asarray(ref_polarizability, dtype=np.float64).reshape(9)).reshape(frames, 3, 3)
    if not jacobian:
        return alpha
    six = slopes.reshape(frames, dofs, 3, 3)[:, :, [r for r, _ in _VEC6], [s for _, s in _VEC6]]  # (S, J, 6)
    rows = np.einsum("tjc,jk->tck", six, folded).reshape(frames, 6, atoms, 3)
    return alpha, rows


def tables_asymmetry(tables: PiecewiseTables) -> float:
    """The largest ``|c[r][s] - c[s][r]|`` of the tables over their largest ``|c|`` (0 for all-zero tables)."""
    c = tables.coefficients.reshape(-1, 3, 3)
    largest = float(np.abs(c).max())
    return float(np.abs(c - c.transpose(0, 2, 1)).max()) / largest if largest > 0 else 0.0


class InterpolationModel(DeviceIncrements, PolarizabilityModel):  # pylint: disable=too-many-instance-attributes
    """A finished interpolation model on GPU ``device``.

    ``ref_structure``: any object with ``lattice``, ``positions``, ``atomic_numbers`` and ``num_atoms``
    (``ramannoodle_amd.structure``); ``ref_polarizability`` ``(3,3)``; ``cart_basis_vectors``: ``J`` arrays ``(N,3)``;
    ``interpolations``: ``J`` ``scipy.interpolate.BSpline`` with values ``(3,3)``, orders 1..5; ``mask`` ``(J,)`` bool,
    ``True`` = the DOF is left out.  ``ValueError`` before any device work: a wrong atom count or DOF count, a model
    without interpolations, an order above 5, non-finite tables.  The entries that use the Jacobian (increments, partial
    and analytic Raman tensors) need symmetric tables and raise ``ValueError`` otherwise."""

    def __init__(self, ref_structure, ref_polarizability, cart_basis_vectors, interpolations, mask=None,
                 device: int = 0) -> None:
        self._ref_structure = ref_structure
        atoms = int(ref_structure.num_atoms)
        self._lattice = np.ascontiguousarray(ref_structure.lattice, dtype=np.float64)
        self._ref_positions = np.ascontiguousarray(ref_structure.positions, dtype=np.float64)
        verify_ndarray_shape("ref_structure.lattice", self._lattice, (3, 3))
        verify_ndarray_shape("ref_structure.positions", self._ref_positions, (atoms, 3))
        ref_polarizability = np.asarray(ref_polarizability)
        verify_ndarray_shape("ref_polarizability", ref_polarizability, (3, 3))
        self._ref_polarizability = np.ascontiguousarray(ref_polarizability, dtype=np.float64)
        self._interpolations = list(interpolations)
        self._tables = piecewise_tables(self._interpolations)
        dofs = len(self._tables.orders)
        vectors = list(cart_basis_vectors)
        if len(vectors) != dofs:
            raise ValueError(f"{len(vectors)} cart_basis_vectors for {dofs} interpolations")
        for j, vector in enumerate(vectors):
            if np.shape(vector) != (atoms, 3):
                raise ValueError(f"cart_basis_vectors[{j}] has wrong shape: {np.shape(vector)} != ({atoms},3): the "
                                 "model and the structure differ in their number of atoms")
        self._basis = np.ascontiguousarray(np.array(vectors, dtype=np.float64).reshape(dofs, atoms, 3))
        for name, array in (("lattice", self._lattice), ("positions", self._ref_positions),
                            ("ref_polarizability", self._ref_polarizability), ("cart_basis_vectors", self._basis)):
            if not np.all(np.isfinite(array)):
                raise ValueError(f"{name} has a non-finite entry")
        self._mask = np.zeros(dofs, dtype=bool)
        if mask is not None:
            self._mask = self._checked_mask(mask)
        self._symmetric = tables_asymmetry(self._tables) <= SYMMETRY_TOLERANCE
        self._device = int(device)
        self._handle = None
        self._mask_on_device = None

    @classmethod
    def from_reference(cls, model, device: int = 0) -> "InterpolationModel":
        """The class swap: any object with ``ref_structure``, ``ref_polarizability``, ``cart_basis_vectors``,
        ``interpolations`` and ``mask`` (the reference's ``InterpolationModel`` and ``ARTModel`` both)."""
        return cls(model.ref_structure, model.ref_polarizability, model.cart_basis_vectors, model.interpolations,
                   mask=model.mask, device=device)

    # ------------------------------------------------------------------ the model as data
    @property
    def num_atoms(self) -> int:
        return self._basis.shape[1]

    @property
    def num_dofs(self) -> int:
        return self._basis.shape[0]

    @property
    def device_index(self) -> int:
        return self._device

    @property
    def ref_lattice(self) -> NDArray[np.float64]:
        return self._lattice.copy()

    @property
    def ref_structure(self):
        return copy.deepcopy(self._ref_structure)

    @property
    def ref_polarizability(self) -> NDArray[np.float64]:
        return self._ref_polarizability.copy()

    @property
    def cart_basis_vectors(self) -> list:
        return [vector.copy() for vector in self._basis]

    @property
    def interpolations(self) -> list:
        return copy.deepcopy(self._interpolations)

    @property
    def tables(self) -> PiecewiseTables:
        return self._tables

    @property
    def is_symmetric(self) -> bool:
        return self._symmetric

    def _checked_mask(self, value) -> NDArray[np.bool_]:
        value = np.asarray(value)
        verify_ndarray_shape("mask", value, (self.num_dofs,))
        return value.astype(bool)

    @property
    def mask(self) -> NDArray[np.bool_]:
        return self._mask.copy()

    @mask.setter
    def mask(self, value) -> None:
        self._mask = self._checked_mask(value)

    def get_masked_model(self, dof_indexes_to_mask) -> "InterpolationModel":
        """A new model (its own device handle) with exactly the DOFs ``dof_indexes_to_mask`` left out."""
        mask = np.zeros(self.num_dofs, dtype=bool)
        mask[dof_indexes_to_mask] = True
        return InterpolationModel(self._ref_structure, self._ref_polarizability, self._basis, self._interpolations,
                                  mask=mask, device=self._device)

    def unmask(self) -> None:
        self._mask = np.zeros(self.num_dofs, dtype=bool)

    def evaluate_host(self, positions_batch, jacobian: bool = False):
        """``evaluate_host`` of this model (numpy, for comparison)."""
        return evaluate_host(self._tables, self._lattice, self._ref_positions, self._ref_polarizability, self._basis,
                             positions_batch, mask=self._mask, jacobian=jacobian)

    # ------------------------------------------------------------------ the device handle
    def _ensure_handle(self):
        lib = _lib.load()
        if self._handle is None:
            handle = C.c_void_p()
            tables = self._tables
            rc = lib.rn_interp_create(self.num_atoms, _ptr(self._lattice), _ptr(self._ref_positions),
                                      _ptr(self._ref_polarizability), self.num_dofs, _ptr(self._basis),
                                      _ptr(tables.piece_offsets), _ptr(tables.breakpoints), _ptr(tables.orders),
                                      _ptr(tables.coefficients), self._device, C.byref(handle))
            _lib.check_interp(rc, None, "rn_interp_create")
            self._handle = handle
            self._mask_on_device = np.zeros(self.num_dofs, dtype=bool)
        if not np.array_equal(self._mask_on_device, self._mask):
            mask = np.ascontiguousarray(self._mask, dtype=np.uint8)
            _lib.check_interp(lib.rn_interp_set_mask(self._handle, _ptr(mask)), self._handle, "rn_interp_set_mask")
            self._mask_on_device = self._mask.copy()
        return self._handle

    def _release(self) -> None:
        handle, self._handle = self._handle, None
        if handle is not None:
            _lib.load().rn_interp_destroy(handle)

    def __del__(self):
        try:
            self._release()
        except Exception:  # pylint: disable=broad-except
            pass

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_handle"] = None
        state["_mask_on_device"] = None
        return state

    # ------------------------------------------------------------------ checks
    @staticmethod
    def _no_lattices(lattices) -> None:
        if lattices is not None:
            raise ValueError("the interpolation model is defined about one cell: it takes no lattices")

    def _need_symmetric(self, what: str) -> None:
        if not self._symmetric:
            raise ValueError(f"{what} uses the Jacobian's six components and needs symmetric tables; this model's "
                             f"asymmetry is {tables_asymmetry(self._tables):.3e} of the largest coefficient")

    @staticmethod
    def _stream(positions) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(positions.device).cuda_stream)

    _partial_raman_entry = "rn_interp_partial_raman_tensors"
    _check_status = staticmethod(_lib.check_interp)

    # ------------------------------------------------------------------ evaluation
    def calc_polarizabilities(self, positions_batch, lattices=None) -> NDArray[np.float64]:
        """Host in, host out: fractional positions ``(S,N,3)`` -> ``(S,3,3)`` (``rn_interp_calc_polarizabilities``)."""
        self._no_lattices(lattices)
        verify_ndarray_shape("positions_batch", positions_batch, (None, self.num_atoms, 3))
        positions = np.ascontiguousarray(positions_batch, dtype=np.float64)
        out = np.empty((positions.shape[0], 3, 3), dtype=np.float64)
        handle = self._ensure_handle()
        rc = _lib.load().rn_interp_calc_polarizabilities(handle, _ptr(positions), positions.shape[0], _ptr(out))
        _lib.check_interp(rc, handle, "rn_interp_calc_polarizabilities")
        return out

    def calc_polarizabilities_device(self, positions, out=None, lattices=None):
        """A contiguous CUDA float64 ``(S,N,3)`` tensor in, a CUDA float64 ``(S,3,3)`` tensor out
        (``rn_interp_forward_device``), enqueued on torch's current stream."""
        self._no_lattices(lattices)
        s = device_frames(positions, self.num_atoms, 1, "the evaluation", self._device)
        out = device_out(out, positions, (s, 3, 3))
        handle = self._ensure_handle()
        rc = _lib.load().rn_interp_forward_device(handle, C.c_void_p(positions.data_ptr()), s,
                                                  C.c_void_p(out.data_ptr()), self._stream(positions))
        _lib.check_interp(rc, handle, "rn_interp_forward_device")
        return out

    def calc_jacobian_device(self, positions, out=None):
        """``d vec6 / d x`` of every frame: a CUDA float64 ``(S,6,N,3)`` tensor (``rn_interp_jacobian_device``)."""
        self._need_symmetric("the Jacobian")
        s = device_frames(positions, self.num_atoms, 1, "the Jacobian", self._device)
        out = device_out(out, positions, (s, 6, self.num_atoms, 3))
        handle = self._ensure_handle()
        rc = _lib.load().rn_interp_jacobian_device(handle, C.c_void_p(positions.data_ptr()), s,
                                                   C.c_void_p(out.data_ptr()), self._stream(positions))
        _lib.check_interp(rc, handle, "rn_interp_jacobian_device")
        return out

    # ------------------------------------------------------------------ phonons
    def _check_raman_arguments(self, ref_positions, displacements, delta, method) -> None:
        raman_arguments(ref_positions, displacements, delta, method, self.num_atoms)

    def calc_raman_tensors(self, ref_positions, displacements, delta: float = RAMAN_TENSOR_CENTRAL_DIFFERENCE,
                           method: str = "finite-difference") -> NDArray[np.float64]:
        """Raman tensors ``(M,3,3)`` of all modes.  ``"finite-difference"`` (the reference's definition):
        ``(alpha(r + delta d_m) - alpha(r - delta d_m)) / delta`` in one batch of the ``2M`` displaced cells;
        ``"analytic"``: ``2 (d alpha / d r) . d_m`` from the Jacobian."""
        self._check_raman_arguments(ref_positions, displacements, delta, method)
        if method == "analytic":
            return self.calc_partial_raman_tensors(ref_positions, displacements,
                                                   np.zeros(self.num_atoms, dtype=np.int64))[:, 0]
        ref = np.asarray(ref_positions, dtype=np.float64)
        eps = np.asarray(displacements, dtype=np.float64) * float(delta)
        alpha = self.calc_polarizabilities(np.concatenate([ref + eps, ref - eps]))
        return (alpha[:len(eps)] - alpha[len(eps):]) / float(delta)

    def calc_partial_raman_tensors(self, ref_positions, displacements, groups) -> NDArray[np.float64]:
        """Raman tensors split by atom group, ``(M,G,3,3)``: ``R[m,g] = 2 sum_{i in g} J_i(ref) . d_{m,i}``
        (``rn_interp_partial_raman_tensors``)."""
        self._check_raman_arguments(ref_positions, displacements, 1.0, "analytic")
        self._need_symmetric("calc_partial_raman_tensors")
        return self._partial_raman_tensors(ref_positions, displacements, groups)

    # ------------------------------------------------------------------ increments along a trajectory
    def calc_group_increments_device(self, positions, groups, out=None, workspace_limit: int = 0, lattices=None):
        """Per-group trapezoid increments along a trajectory (``rn_interp_group_increments_device``): CUDA float64
        ``(S,N,3)`` in, ``(S-1,G,3,3)`` out, as ``PotGNN.calc_group_increments_device`` for a fixed cell."""
        self._no_lattices(lattices)
        self._need_symmetric("calc_group_increments_device")
        s = device_frames(positions, self.num_atoms, 2, "group increments", self._device)
        labels, num_groups = self._group_labels(groups)
        out = device_out(out, positions, (s - 1, num_groups, 3, 3))
        handle = self._ensure_handle()
        rc = _lib.load().rn_interp_group_increments_device(
            handle, C.c_void_p(positions.data_ptr()), s, _ptr(labels), num_groups, int(workspace_limit),
            C.c_void_p(out.data_ptr()), self._stream(positions))
        _lib.check_interp(rc, handle, "rn_interp_group_increments_device")
        return out

    def calc_group_increments(self, positions_ts, groups, lattices=None) -> NDArray[np.float64]:
        """``calc_group_increments_device`` for host arrays."""
        self._no_lattices(lattices)
        return self._increments_from_host(self.calc_group_increments_device, positions_ts, None, groups)

    def calc_mode_increments_device(self, positions, displacements, projectors, rest: bool = True, out=None,
                                    workspace_limit: int = 0, lattices=None):
        """Per-mode trapezoid increments along a trajectory (``rn_interp_mode_increments_device``): CUDA float64
        ``(S,N,3)`` in, ``(S-1,M+rest,3,3)`` out, as ``PotGNN.calc_mode_increments_device`` for a fixed cell."""
        self._no_lattices(lattices)
        self._need_symmetric("calc_mode_increments_device")
        s = device_frames(positions, self.num_atoms, 2, "mode increments", self._device)
        disp, proj = mode_arrays(displacements, projectors, self.num_atoms)
        out = device_out(out, positions, (s - 1, disp.shape[0] + bool(rest), 3, 3))
        handle = self._ensure_handle()
        rc = _lib.load().rn_interp_mode_increments_device(
            handle, C.c_void_p(positions.data_ptr()), s, _ptr(disp), _ptr(proj), disp.shape[0], int(bool(rest)),
            int(workspace_limit), C.c_void_p(out.data_ptr()), self._stream(positions))
        _lib.check_interp(rc, handle, "rn_interp_mode_increments_device")
        return out

    def calc_mode_increments(self, positions_ts, displacements, projectors, rest: bool = True,
                             lattices=None) -> NDArray[np.float64]:
        """``calc_mode_increments_device`` for host arrays."""
        self._no_lattices(lattices)
        return self._increments_from_host(self.calc_mode_increments_device, positions_ts, None, displacements,
                                          projectors, rest=rest)
