"""Distances to a reference set and farthest-point selection of rows of descriptors (an addition): how far a frame lies
from the frames a model was trained on, and which frames to label next.

Definition.  All float64.  ``X`` ``(S,D)``: the rows to judge; ``R`` ``(M,D)``: the reference rows; ``center`` and
``scale`` ``(D,)``: optional (zeros, ones).  ``d2(a, b) = sum_c ((a_c - b_c) scale_c)^2``: ``center`` cancels in a
difference and only moves the origin of the products the device search forms.

* ``nearest``: ``index[s] = argmin_j d2(X_s, R_j)``, the lowest ``j`` among equal values, and ``distance[s] =
  sqrt(d2(X_s, R_index[s]))``.  With ``exclude_self`` row ``s`` ignores ``j = s`` (for ``X`` = ``R``: the leave-one-out
  neighbour).  A row without any candidate (``M = 1`` with ``exclude_self``) gets index -1 and an infinite distance.
* ``select_farthest``: ``mind[s]`` starts from the squared nearest distance to ``R`` when there is a reference, from
  +inf when there is none.  Pick ``k``: ``p_k = argmax_s mind[s]`` over the rows not picked yet, the lowest ``s`` among
  equal values; ``distance[k] = sqrt(mind[p_k])``; then ``mind[s] = min(mind[s], d2(X_s, X_p_k))``.  Without a reference
  the first pick is ``first`` or, by default, the row farthest from the column mean of ``X`` (the lowest ``s`` among
  equal values), and its distance is infinite.  ``first`` with a reference is refused: the reference decides.

``nearest_host`` and ``select_farthest_host`` state this in numpy; ``nearest`` and ``select_farthest`` with a ``device``
(or with CUDA tensors, which are read where they are) compute it on the GPU (``include/rn_select.h``), differing by the
order of the sums only; with ``device=None`` and host arrays they are the host functions.  Every ``ValueError`` comes
before any device work.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.typing import NDArray

from ramannoodle_amd._source import is_tensor, source

_TENSOR_REFUSAL = "a tensor of rows must be a contiguous float64 CUDA tensor"


def _rows(name: str, value, columns: int | None = None, minimum: int = 0) -> NDArray[np.float64]:
    rows = np.asarray(value)
    if rows.dtype.kind not in "iuf" or rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError(f"{name} must be a real array (rows, D) with D >= 1, not {rows.dtype} {rows.shape}")
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if columns is not None and rows.shape[1] != columns:
        raise ValueError(f"{name} has D = {rows.shape[1]} columns, the rows to judge have {columns}")
    if rows.shape[0] < minimum:
        raise ValueError(f"{name} must hold at least {minimum} row(s)")
    bad = np.argwhere(~np.isfinite(rows))
    if len(bad):
        raise ValueError(f"{name}[{bad[0][0]}][{bad[0][1]}] is not finite")
    return rows


def _column_vector(name: str, value, columns: int) -> NDArray[np.float64] | None:
    if value is None:
        return None
    vector = np.asarray(value.detach().cpu().numpy() if is_tensor(value) else value)
    if vector.dtype.kind not in "iuf" or vector.shape != (columns,):
        raise ValueError(f"{name} must hold D = {columns} reals, not {vector.dtype} {vector.shape}")
    vector = np.ascontiguousarray(vector, dtype=np.float64)
    bad = np.flatnonzero(~np.isfinite(vector))
    if len(bad):
        raise ValueError(f"{name}[{bad[0]}] is not finite")
    return vector


def _count_and_first(count, first, rows: int, with_reference: bool) -> tuple[int, int]:
    if isinstance(count, (bool, np.bool_)) or not isinstance(count, (int, np.integer)) or count < 0:
        raise ValueError(f"count = {count!r} must be a non-negative integer")
    if count > rows:
        raise ValueError(f"count = {count} picks of S = {rows} rows")
    if first is None:
        return int(count), -1
    if isinstance(first, (bool, np.bool_)) or not isinstance(first, (int, np.integer)) or not 0 <= first < rows:
        raise ValueError(f"first = {first!r} is not a row of S = {rows}")
    if with_reference:
        raise ValueError("first is for a selection without a reference set: the reference decides the first pick")
    return int(count), int(first)


def _squared_distances(rows, point, scale):
    difference = rows - point
    if scale is not None:
        difference = difference * scale
    return np.einsum("sc,sc->s", difference, difference)


def nearest_host(descriptors, reference, center=None, scale=None, exclude_self: bool = False):
    """``(distance (S,), index (S,) int64)`` of the module's definition, in numpy from differences: the statement the
    device path is tested against.  ``center`` is checked and otherwise without effect."""
    rows = _rows("descriptors", descriptors)
    others = _rows("reference", reference, rows.shape[1], minimum=1)
    _column_vector("center", center, rows.shape[1])
    scale = _column_vector("scale", scale, rows.shape[1])
    squared = np.full(len(rows), np.inf)
    index = np.full(len(rows), -1, dtype=np.int64)
    for s, row in enumerate(rows):
        candidates = _squared_distances(others, row, scale)
        if exclude_self and s < len(others):
            candidates[s] = np.inf
        j = int(np.argmin(candidates))  # (the first of equal values)
        if np.isfinite(candidates[j]):
            squared[s], index[s] = candidates[j], j
    return np.sqrt(squared), index


def select_farthest_host(descriptors, count, reference=None, first=None, center=None, scale=None):
    """``(indices (count,) int64, distances (count,))`` of the module's definition, in numpy."""
    rows = _rows("descriptors", descriptors)
    others = None if reference is None else _rows("reference", reference, rows.shape[1])
    with_reference = others is not None and len(others) > 0
    count, first = _count_and_first(count, first, len(rows), with_reference)
    _column_vector("center", center, rows.shape[1])
    scale = _column_vector("scale", scale, rows.shape[1])
    picks = np.zeros(count, dtype=np.int64)
    squared = np.zeros(count)
    if count == 0:
        return picks, squared
    if with_reference:
        mind = np.array([_squared_distances(others, row, scale).min() for row in rows])
    else:
        mind = np.full(len(rows), np.inf)
        if first < 0:
            first = int(np.argmax(_squared_distances(rows, rows.mean(axis=0), scale)))
    picked = np.zeros(len(rows), dtype=bool)
    for k in range(count):
        if k == 0 and not with_reference:
            pick = first
        else:
            pick = int(np.argmax(np.where(picked, -1.0, mind)))  # (the first of equal values)
        picks[k], squared[k] = pick, mind[pick]
        picked[pick] = True
        mind = np.minimum(mind, _squared_distances(rows, rows[pick], scale))
    return picks, np.sqrt(squared)


def _operand(name: str, value, columns: int | None = None, minimum: int = 0):
    """``(pointer, rows, columns, device index or None, stream or None, keepalive)`` of a host array or a CUDA tensor."""
    if not is_tensor(value):
        rows = _rows(name, value, columns, minimum)
        return rows.ctypes.data, rows.shape[0], rows.shape[1], None, None, rows
    pointer, device, stream, keep = source(value, _TENSOR_REFUSAL)
    if value.dim() != 2 or value.shape[1] < 1:
        raise ValueError(f"{name} must be (rows, D) with D >= 1, not {tuple(value.shape)}")
    if columns is not None and value.shape[1] != columns:
        raise ValueError(f"{name} has D = {value.shape[1]} columns, the rows to judge have {columns}")
    if value.shape[0] < minimum:
        raise ValueError(f"{name} must hold at least {minimum} row(s)")
    return pointer, int(value.shape[0]), int(value.shape[1]), device, stream, keep


def _placement(x, r, device):
    """The GPU and the stream of a call, ``stream`` ``None`` for host arrays: tensors and arrays do not mix."""
    x_device, r_device = x[3], None if r is None else r[3]
    if r is not None and (x_device is None) != (r_device is None):
        raise ValueError("descriptors and reference must both be host arrays or both be CUDA tensors")
    if x_device is None:
        return device, None
    if r_device is not None and r_device != x_device:
        raise ValueError(f"descriptors are on GPU {x_device}, the reference is on GPU {r_device}")
    if device is not None and int(device) != x_device:
        raise ValueError(f"device = {device}, the tensors are on GPU {x_device}")
    return x_device, x[4]


def _pointer(array):
    return C.c_void_p(None if array is None else array.ctypes.data)


def nearest(descriptors, reference, center=None, scale=None, exclude_self: bool = False, device: int | None = None):
    """``(distance (S,), index (S,) int64)``: per row of ``descriptors`` the Euclidean distance to its nearest row of
    ``reference`` and that row's index, as host arrays.  ``descriptors`` and ``reference``: host arrays, computed on
    GPU ``device`` (``rn_select_nearest``) or, with ``device=None``, by ``nearest_host``; or contiguous float64 CUDA
    tensors, read where they are, ordered after torch's current stream (``rn_select_nearest_device``)."""
    if device is None and not is_tensor(descriptors) and not is_tensor(reference):
        return nearest_host(descriptors, reference, center, scale, exclude_self)
    from ramannoodle_amd import _lib
    x = _operand("descriptors", descriptors)
    r = _operand("reference", reference, x[2], minimum=1)
    device, stream = _placement(x, r, device)
    center, scale = _column_vector("center", center, x[2]), _column_vector("scale", scale, x[2])
    squared = np.empty(x[1], dtype=np.float64)
    index = np.empty(x[1], dtype=np.int64)
    lib = _lib.load()
    entry = lib.rn_select_nearest if stream is None else lib.rn_select_nearest_device
    tail = () if stream is None else (C.c_void_p(stream),)
    rc = entry(int(device), C.c_void_p(x[0]), x[1], C.c_void_p(r[0]), r[1], x[2], _pointer(center), _pointer(scale),
               int(bool(exclude_self)), _pointer(squared), _pointer(index), *tail)
    _lib.check_status(rc, "rn_select_nearest", "rn_select_last_error")
    return np.sqrt(squared), index


def select_farthest(descriptors, count, reference=None, first=None, center=None, scale=None, device: int | None = None):
    """``(indices (count,) int64, distances (count,))``: greedy farthest-point selection of ``count`` rows of
    ``descriptors``, seeded with ``reference`` when it is given, as host arrays.  Host arrays or CUDA tensors as for
    ``nearest`` (``rn_select_farthest``, ``rn_select_farthest_device``)."""
    if device is None and not is_tensor(descriptors) and not is_tensor(reference):
        return select_farthest_host(descriptors, count, reference, first, center, scale)
    from ramannoodle_amd import _lib
    x = _operand("descriptors", descriptors)
    r = None if reference is None else _operand("reference", reference, x[2])
    device, stream = _placement(x, r, device)
    references = 0 if r is None else r[1]
    count, first = _count_and_first(count, first, x[1], references > 0)
    center, scale = _column_vector("center", center, x[2]), _column_vector("scale", scale, x[2])
    picks = np.empty(count, dtype=np.int64)
    squared = np.empty(count, dtype=np.float64)
    lib = _lib.load()
    entry = lib.rn_select_farthest if stream is None else lib.rn_select_farthest_device
    tail = () if stream is None else (C.c_void_p(stream),)
    rc = entry(int(device), C.c_void_p(x[0]), x[1], x[2], C.c_void_p(r[0] if references else None), references,
               _pointer(center), _pointer(scale), first, count, _pointer(picks), _pointer(squared), *tail)
    _lib.check_status(rc, "rn_select_farthest", "rn_select_last_error")
    return picks, np.sqrt(squared)


def tile_rows() -> int:
    """The rows of a tile of the device search (``rn_select_tile_rows``)."""
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_select_tile_rows())


def reference_splits(rows: int, references: int) -> int:
    """The ascending ranges the device search splits ``references`` rows into for ``rows`` rows to judge."""
    from ramannoodle_amd import _lib
    return int(_lib.load().rn_select_reference_splits(int(rows), int(references)))


class DomainCheck:
    """Was the model inside its training domain?  Holds the structure descriptors of the training frames
    (``PotGNN.calc_descriptors``) and measures new frames against them in the model's own latent space.

    * ``center`` is the column mean of the training descriptors and ``scale`` is ``1 / std`` of each column (the
      population standard deviation); a constant column (``std <= 1e-12 max(1, |mean|)``) gets scale 1.
    * ``unit`` is the ``quantile`` of the leave-one-out nearest distances of the training frames among themselves, in
      those scaled coordinates.  ``quantile`` is a definition with a default, not a measured number: at 0.95 one
      training frame in twenty would itself count as outside.
    * ``novelty`` of a frame is its distance to the nearest training frame divided by ``unit``; ``outside`` is
      ``novelty > 1``; ``select`` picks the frames to label next, farthest-point selection seeded with the training set.

    ``training_positions``: host ``(M,N,3)`` fractional positions, or a contiguous float64 CUDA tensor, with ``M >= 2``;
    ``lattices``: one cell per frame, as for ``calc_descriptors``.  Frames given as CUDA tensors are described, searched
    and selected in HBM: only distances and indices, ``center`` and ``scale`` reach the host."""

    def __init__(self, model, training_positions, lattices=None, quantile: float = 0.95):
        if not 0.0 < float(quantile) <= 1.0:
            raise ValueError(f"quantile = {quantile!r} must lie in (0, 1]")
        self._model = model
        self._references = {}
        self._native = False  # are the training descriptors a CUDA tensor
        reference = self._describe(training_positions, lattices)
        if reference.shape[0] < 2:
            raise ValueError("the training set must hold at least 2 frames: a leave-one-out distance needs a neighbour")
        self._native = is_tensor(reference)
        self._references[self._native] = reference
        if is_tensor(reference):
            mean = reference.mean(dim=0).cpu().numpy()
            std = reference.std(dim=0, unbiased=False).cpu().numpy()
        else:
            mean, std = reference.mean(axis=0), reference.std(axis=0)
        constant = std <= 1e-12 * np.maximum(1.0, np.abs(mean))
        self.center = np.ascontiguousarray(mean, dtype=np.float64)
        self.scale = np.where(constant, 1.0, 1.0 / np.where(constant, 1.0, std))
        self.quantile = float(quantile)
        self.training_distances = nearest(reference, reference, self.center, self.scale, exclude_self=True,
                                          device=self._device(reference))[0]
        self.unit = float(np.quantile(self.training_distances, self.quantile))
        if not self.unit > 0.0:
            raise ValueError("the training frames' leave-one-out distances have a zero quantile: duplicated frames")

    def _device(self, rows):
        return None if is_tensor(rows) else self._model.device_index

    def _describe(self, positions, lattices=None):
        if hasattr(positions, "get_descriptors"):  # a Trajectory or a TrajectoryEnsemble: its own cells
            if lattices is not None:
                raise ValueError("a trajectory carries its own lattices")
            return positions.get_descriptors(self._model, on_device=self._native)
        if is_tensor(positions):
            return self._model.calc_descriptors_device(positions, lattices=lattices)
        return self._model.calc_descriptors(positions, lattices=lattices)

    def _reference_for(self, rows):
        """The training descriptors where ``rows`` are: a host array, or a CUDA tensor."""
        tensor = is_tensor(rows)
        if tensor not in self._references:
            other = self._references[not tensor]
            if tensor:
                import torch
                self._references[True] = torch.tensor(other, dtype=torch.float64, device=rows.device)
            else:
                self._references[False] = other.cpu().numpy()
        return self._references[tensor]

    @property
    def training_descriptors(self):
        """The training frames' descriptors ``(M, D)``, as they were computed: a host array or a CUDA tensor."""
        return self._references[self._native]

    def novelty(self, positions, lattices=None) -> NDArray[np.float64]:
        """Per frame of ``positions`` (host, CUDA tensor, or a ``Trajectory``): the distance to the nearest training
        frame in units of ``unit``."""
        rows = self._describe(positions, lattices)
        distance = nearest(rows, self._reference_for(rows), self.center, self.scale, device=self._device(rows))[0]
        return distance / self.unit

    def outside(self, positions, lattices=None) -> NDArray[np.bool_]:
        """``novelty > 1``: the frames farther from the training set than ``quantile`` of it is from itself."""
        return self.novelty(positions, lattices) > 1.0

    def select(self, positions, count: int, lattices=None) -> NDArray[np.int64]:
        """The ``count`` frames of ``positions`` to label next: farthest-point selection seeded with the training set, so
        that a frame the training set already holds comes last."""
        rows = self._describe(positions, lattices)
        return select_farthest(rows, count, reference=self._reference_for(rows), center=self.center, scale=self.scale,
                               device=self._device(rows))[0]
