"""PotGNN polarizability model evaluated by hand-written gfx950 kernels.

Host-side mirror of ``ramannoodle.pmodel.torch.PotGNN`` (``ramannoodle/pmodel/torch/
_gnn.py:418-721``) for the evaluation path: same constructor signature and error
messages, same ``state_dict`` keys, ``forward`` / ``calc_polarizabilities`` with the same
argument meaning.  All arithmetic on positions happens on the device through the C ABI
in ``include/rn_potgnn.h``; PyTorch is used only to hold parameter tensors and device
buffers.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch
from numpy.typing import NDArray
from torch.autograd.function import once_differentiable

from ramannoodle_amd import _lib
from ramannoodle_amd.abstract import PolarizabilityModel
from ramannoodle_amd.constants import RAMAN_TENSOR_CENTRAL_DIFFERENCE
from ramannoodle_amd.exceptions import verify_ndarray_shape
from ramannoodle_amd.pmodel import graph as graph_utils
from ramannoodle_amd.pmodel._device import (DeviceIncrements, _ptr, check_out as _check_out, device_frames, device_out,
                                            mode_arrays, raman_arguments)

_VEC_TO_TENSOR = np.array([[0, 3, 4], [3, 1, 5], [4, 5, 2]])  # dataset/torch/utils.py:30-37


def polarizability_vectors_to_tensors(vectors):
    """``[S,6] (xx,yy,zz,xy,xz,yz) -> [S,3,3]`` (``dataset/torch/utils.py:20-41``)."""
    if vectors.ndim != 2 or vectors.shape[1] != 6:
        raise ValueError(f"polarizability_vectors has wrong size: {list(vectors.shape)} != [_,6]")
    return vectors[:, _VEC_TO_TENSOR]


def polarizability_tensors_to_vectors(tensors):
    """``[S,3,3] -> [S,6]`` (``dataset/torch/utils.py:44-60``)."""
    if tensors.ndim != 3 or tuple(tensors.shape[1:]) != (3, 3):
        raise ValueError(f"polarizability_tensors has wrong size: {list(tensors.shape)} != [_,3,3]")
    return tensors[:, [0, 1, 2, 0, 0, 1], [0, 1, 2, 1, 2, 2]]


def _wants_float64(dtype) -> bool:
    """Evaluation dtype selector: ``None`` = torch's default dtype (``_gnn.py:705``)."""
    if dtype is None:
        dtype = torch.get_default_dtype()
    if dtype in (torch.float64, np.float64, float, "float64", "f64"):
        return True
    if dtype in (torch.float32, np.float32, "float32", "f32"):
        return False
    raise ValueError(f"unsupported evaluation dtype: {dtype}")


_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_void_p)


class _Activation(torch.nn.Module):
    """Placeholder for the reference's parameter-free ``ShiftedSoftplus`` entries of its ``Sequential`` containers
    (``_gnn.py:508-514, 532-539``): keeps the children's indices -- and with them the ``state_dict`` keys -- the
    reference's.  The arithmetic happens in the kernels."""

    def forward(self, x):  # pylint: disable=missing-function-docstring
        return torch.nn.functional.softplus(x) - 0.6931471805599453


class _GaussianFilter(torch.nn.Module):
    """Holder of the ``offset`` buffer (``_gnn.py:53-66``)."""

    def __init__(self, start: float, end: float, steps: int):
        super().__init__()
        self.register_buffer("offset", torch.linspace(start, end, steps, dtype=torch.float32))


class _NodeBlockParams(torch.nn.Module):
    """Parameters of ``_NodeBlock`` under the reference's names, in its order (``_gnn.py:106-120``)."""

    def __init__(self, fn: int, fe: int):
        super().__init__()
        self.c1_linear = torch.nn.Linear(fn + fe, 2 * fn)
        self.c1_norm = torch.nn.LayerNorm(2 * fn)
        self.final_norm = torch.nn.LayerNorm(fn)


class _EdgeBlockParams(torch.nn.Module):
    """Parameters of ``_EdgeBlock`` under the reference's names, in its order (``_gnn.py:180-205``)."""

    def __init__(self, fn: int, fe: int):
        super().__init__()
        self.c2_linear = torch.nn.Linear(fn, 2 * fe)
        self.c3_linear = torch.nn.Linear(3 * fn + 2 * fe, 2 * fe)
        self.c2_norm_1 = torch.nn.LayerNorm(2 * fe)
        self.c3_norm_1 = torch.nn.LayerNorm(2 * fe)
        self.c2_norm_2 = torch.nn.LayerNorm(fe)
        self.c3_norm_2 = torch.nn.LayerNorm(fe)


class PotGNN(torch.nn.Module, DeviceIncrements, PolarizabilityModel):  # pylint: disable=too-many-instance-attributes
    """POlarizability Tensor Graph Neural Network, device evaluation.

    A ``torch.nn.Module`` like the reference's (``_gnn.py:418-421``): its children are the reference's containers
    (``_node_embedding``, ``_edge_embedding``, ``_node_blocks``, ``_edge_blocks``, ``_to_polarizability_embedding``)
    holding real ``Linear`` / ``Embedding`` / ``LayerNorm`` / ``BatchNorm1d`` modules, so ``parameters()``,
    ``state_dict()``, ``apply()``, ``modules()``, hooks, ``model(...)``, ``torch.save(model)`` and ``.to()`` are torch's
    own.  The children only HOLD the parameters: ``forward`` hands them to the device kernels.

    Parameters are positional-compatible with the reference
    (``_gnn.py:453-464``); ``device`` (HIP ordinal) and ``max_chunk_structures`` are
    additions.  ``ref_structure`` only needs ``lattice``, ``positions``,
    ``atomic_numbers`` and ``num_atoms``.
    """

    # pylint: disable=too-many-arguments,too-many-positional-arguments,too-many-locals
    def __init__(self, ref_structure, cutoff: float, size_node_embedding: int,
                 size_edge_embedding: int, num_message_passes: int,
                 gaussian_filter_start: float, gaussian_filter_end: float,
                 mean_polarizability: NDArray[np.float64],
                 stddev_polarizability: NDArray[np.float64], device: int | None = None,
                 max_chunk_structures: int = 0):
        if cutoff <= 0:
            raise ValueError(f"invalid cutoff: {cutoff} <= 0")
        if size_node_embedding <= 0:
            raise ValueError(f"invalid size_node_embedding: {size_node_embedding} <= 0")
        if size_edge_embedding <= 0:
            raise ValueError(f"invalid size_edge_embedding: {size_edge_embedding} <= 0")
        if num_message_passes <= 0:
            raise ValueError(f"invalid num_message_passes: {num_message_passes} <= 0")
        if gaussian_filter_start < 0:
            raise ValueError(f"invalid gaussian_filter_start: {gaussian_filter_start} < 0")
        if gaussian_filter_end <= gaussian_filter_start:
            raise ValueError(
                f"invalid gaussian_filter_end: {gaussian_filter_end} <= gaussian_filter_start")
        verify_ndarray_shape("mean_polarizability", mean_polarizability, (3, 3))
        verify_ndarray_shape("stddev_polarizability", stddev_polarizability, (3, 3))
        _lib.load()  # fail loudly before any work if the HIP library is absent
        torch.nn.Module.__init__(self)

        self._ref_structure = ref_structure
        self._cutoff = cutoff
        self._fn = int(size_node_embedding)
        self._fe = int(size_edge_embedding)
        self._passes = int(num_message_passes)
        self._mean_polarizability = np.array(mean_polarizability, dtype=np.float64)
        self._stddev_polarizability = np.array(stddev_polarizability, dtype=np.float64)
        self._device = device
        self._max_chunk = int(max_chunk_structures)

        # frozen graph of the reference structure (_gnn.py:489-499)
        # (pair test on the device when there is one; the numpy restatement of the same float32
        # arithmetic serves GPU-less hosts, e.g. unit tests -- both are pinned by the fixtures)
        if torch.cuda.is_available():
            dev = device if device is not None else torch.cuda.current_device()
            edges = graph_utils.radius_graph_pbc_device(ref_structure.lattice, ref_structure.positions,
                                                        cutoff, dev)
        else:
            edges = graph_utils.radius_graph_pbc(ref_structure.lattice, ref_structure.positions, cutoff)
        self._ref_edge_indexes = np.vstack([np.zeros((1, edges.shape[1]), dtype=np.int64), edges])
        self._atom_type_map = graph_utils.atom_type_map(ref_structure.atomic_numbers)
        self._num_atom_types = int((self._atom_type_map >= 0).sum())

        self._gaussian_filter = (float(gaussian_filter_start), float(gaussian_filter_end))
        if self._fe < 2:
            raise ValueError("invalid size_edge_embedding: the Gaussian filter needs >= 2 steps")
        # the reference's module tree, created in its order so that the same torch.manual_seed gives the same initial
        # weights (_gnn.py:508-539): trainable entries are Parameters (torch.optim works on them), the Gaussian offsets
        # and the BatchNorm running statistics are buffers
        fn, fe, k = self._fn, self._fe, self._num_atom_types
        self._node_embedding = torch.nn.Sequential(torch.nn.Embedding(k, fn), _Activation(), torch.nn.Linear(fn, fn),
                                                   _Activation(), torch.nn.Linear(fn, fn))
        self._edge_embedding = _GaussianFilter(*self._gaussian_filter, fe)
        self._node_blocks = torch.nn.ModuleList(_NodeBlockParams(fn, fe) for _ in range(self._passes))
        self._edge_blocks = torch.nn.ModuleList(_EdgeBlockParams(fn, fe) for _ in range(self._passes))
        self._to_polarizability_embedding = torch.nn.Sequential(
            torch.nn.Linear(fe, fe), torch.nn.BatchNorm1d(fe), _Activation(), torch.nn.Linear(fe, fe), _Activation(),
            torch.nn.Linear(fe, 12))
        offset = self._edge_embedding.offset
        self._gauss_coefficient = -0.5 / (float(offset[1]) - float(offset[0])) ** 2  # _gnn.py:64
        self._device_ahead = False     # DeviceAdam stepped: the device weights are newer than the host tensors
        self._device_training = False  # gradients / optimiser state / BatchNorm buffers live in HBM
        self._device_anchor = torch.zeros(1, requires_grad=True)
        self._device_batches_tracked = 0
        self._handle = None
        self._profiling = 0
        self._uploaded_version = None
        # (a fresh torch Module is in training mode; calc_polarizabilities switches to eval)

    @property
    def _state_store(self) -> "OrderedDict[str, torch.Tensor]":
        """The module's own parameters and buffers, by ``state_dict`` key and in its order (the tensors themselves)."""
        return torch.nn.Module.state_dict(self, keep_vars=True)

    @property
    def _state(self) -> "OrderedDict[str, torch.Tensor]":
        """The module's parameters and buffers by ``state_dict`` key (the tensors themselves), refreshed from the device
        first when a device-resident optimiser has moved the weights (``DeviceAdam``)."""
        if self._device_ahead:
            self._sync_from_device()
        return self._state_store

    def _sync_from_device(self) -> None:
        store = self._state_store
        blob = np.empty(sum(v.numel() for v in store.values() if v.is_floating_point()), dtype=np.float32)
        rc = _lib.load().rn_potgnn_get_weights(self._handle, _ptr(blob), blob.size)
        _lib.check(rc, self._handle, "rn_potgnn_get_weights")
        offset = 0
        with torch.no_grad():
            for value in store.values():
                if value.is_floating_point():
                    n = value.numel()
                    value.copy_(torch.from_numpy(blob[offset:offset + n].reshape(tuple(value.shape))).to(value.device))
                    offset += n
            store["_to_polarizability_embedding.1.num_batches_tracked"].fill_(self._device_batches_tracked)
        self._device_ahead = False
        self._uploaded_version = sum(int(v._version) for v in store.values())  # device == host again

    def reset_parameters(self) -> None:
        """Re-initialise every parameter and buffer (``_gnn.py:559-566``: ``reset`` on every child, in order)."""
        if self._device_ahead:
            self._sync_from_device()
        for module in self.modules():
            if module is not self and hasattr(module, "reset_parameters"):
                module.reset_parameters()
        with torch.no_grad():
            self._edge_embedding.offset.copy_(torch.linspace(*self._gaussian_filter, self._fe, dtype=torch.float32))

    # ------------------------------------------------------------------ properties
    @property
    def ref_edge_indexes(self) -> np.ndarray:
        """``int64[3,E]`` (graph, a, b) as ``PotGNN._ref_edge_indexes`` (_gnn.py:492)."""
        return self._ref_edge_indexes.copy()

    @property
    def num_edges(self) -> int:
        return int(self._ref_edge_indexes.shape[1])

    @property
    def ref_lattice(self) -> np.ndarray:
        """The lattice of the reference structure, float64 ``(3,3)`` (rows = lattice vectors; a copy)."""
        return np.array(self._ref_structure.lattice, dtype=np.float64)

    @property
    def num_atoms(self) -> int:
        return int(self._ref_structure.num_atoms)

    @property
    def atom_type_map(self) -> np.ndarray:
        return self._atom_type_map.copy()

    @property
    def gauss_coefficient(self) -> float:
        return self._gauss_coefficient

    # ------------------------------------------------------------------ parameters
    _BUFFER_SUFFIXES = ("_edge_embedding.offset", "running_mean", "running_var", "num_batches_tracked")

    @classmethod
    def _is_trainable(cls, key: str) -> bool:
        return not key.endswith(cls._BUFFER_SUFFIXES)

    # torch.nn.Module's own parameters / named_parameters / state_dict / load_state_dict / apply / train / eval, with one
    # addition: after a device-resident optimiser step the host tensors are refreshed from the device first
    def _fresh(self) -> None:
        if self._device_ahead:
            self._sync_from_device()

    def parameters(self, recurse: bool = True):  # pylint: disable=missing-function-docstring
        self._fresh()
        return super().parameters(recurse)

    def named_parameters(self, *args, **kwargs):  # pylint: disable=missing-function-docstring
        self._fresh()
        return super().named_parameters(*args, **kwargs)

    def state_dict(self, *args, **kwargs):
        """Same keys, shapes and order as the reference's ``state_dict()``."""
        self._fresh()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """``torch.nn.Module.load_state_dict`` (numpy arrays are accepted as values too); the Parameter objects stay the
        same, so optimisers holding them stay valid."""
        self._fresh()
        state = OrderedDict((k, v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))) for k, v in state_dict.items())
        return super().load_state_dict(state, strict=strict, assign=assign)

    # ------------------------------------------------------------------ device handle
    def _weights_blob(self) -> np.ndarray:
        parts = [v.detach().cpu().numpy().astype(np.float32).ravel() for v in self._state.values()
                 if v.is_floating_point()]
        return np.ascontiguousarray(np.concatenate(parts))

    def _version(self) -> int:
        return sum(int(v._version) for v in self._state.values())  # bumped by in-place updates

    def _ensure_handle(self):
        if self._handle is not None:
            if self._device_ahead:  # the device copy is the current one (see the _state property)
                return self._handle
            if self._uploaded_version != self._version():  # e.g. after optimizer.step()
                blob = self._weights_blob()
                rc = _lib.load().rn_potgnn_set_weights(self._handle, _ptr(blob), blob.size)
                _lib.check(rc, self._handle, "rn_potgnn_set_weights")
                self._uploaded_version = self._version()
            return self._handle
        lib = _lib.load()
        device = self._device
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        cfg = _lib.Config(self.num_atoms, self.num_edges, self._num_atom_types, self._fn, self._fe,
                          self._passes, self._gauss_coefficient, self._max_chunk, int(device))
        blob = self._weights_blob()
        expected = lib.rn_potgnn_weight_count(C.byref(cfg))
        if blob.size != expected:
            raise RuntimeError(f"weight blob has {blob.size} floats, library expects {expected}")
        edge_a = np.ascontiguousarray(self._ref_edge_indexes[1], dtype=np.int32)
        edge_b = np.ascontiguousarray(self._ref_edge_indexes[2], dtype=np.int32)
        types = np.ascontiguousarray(
            self._atom_type_map[np.asarray(self._ref_structure.atomic_numbers)], dtype=np.int32)
        lattice = np.ascontiguousarray(self._ref_structure.lattice, dtype=np.float64)
        mean = np.ascontiguousarray(self._mean_polarizability)
        std = np.ascontiguousarray(self._stddev_polarizability)
        handle = C.c_void_p()
        rc = lib.rn_potgnn_create(C.byref(cfg), _ptr(edge_a), _ptr(edge_b), _ptr(types),
                                  _ptr(lattice), _ptr(blob), blob.size, _ptr(mean), _ptr(std),
                                  C.byref(handle))
        _lib.check(rc, None, "rn_potgnn_create")
        self._handle = handle
        self._uploaded_version = self._version()
        if self._profiling:
            lib.rn_potgnn_set_profiling(handle, self._profiling)
        return handle

    # -- copies and pickles carry the host state only (copy.deepcopy(model), torch.save(model)): the
    #    device handle, its optimiser state and the data-parallel hooks belong to this object
    def __getstate__(self):
        self._fresh()  # (the host tensors are fetched from the device first when that copy is ahead)
        state = dict(self.__dict__)
        for key in ("_handle", "_dp_group", "_dp_callback", "_dp_installed_on"):
            state.pop(key, None)
        state.update(_device_ahead=False, _device_training=False, _uploaded_version=None)
        return state

    def __setstate__(self, state):
        torch.nn.Module.__setstate__(self, state)
        self.__dict__["_handle"] = None

    def _release(self) -> None:
        if getattr(self, "_handle", None) is not None:
            _lib.load().rn_potgnn_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:  # pylint: disable=broad-except
            pass

    # ------------------------------------------------------------------ evaluation
    def _check_positions(self, positions_batch) -> np.ndarray:
        verify_ndarray_shape("positions_batch", positions_batch, (None, self.num_atoms, 3))
        return np.ascontiguousarray(positions_batch, dtype=np.float64)

    def _check_lattices(self, lattices, frames: int) -> np.ndarray:
        """Host lattices of a variable-cell call: ``(S,3,3)``, one per frame, as contiguous float64.  Their values (finite,
        non-singular) are checked by the library before any device work."""
        verify_ndarray_shape("lattices", lattices, (frames, 3, 3))
        return np.ascontiguousarray(lattices, dtype=np.float64)

    def _check_device_lattices(self, lattices, positions: torch.Tensor) -> torch.Tensor:
        """Device lattices of a variable-cell call: a contiguous float64 ``(S,3,3)`` tensor next to the positions.  Their
        values are not inspected (that would wait for the device): a non-finite lattice gives a non-finite result."""
        if not (isinstance(lattices, torch.Tensor) and lattices.is_cuda and lattices.dtype == torch.float64
                and lattices.is_contiguous()):
            raise ValueError("lattices must be a contiguous float64 device tensor")
        if lattices.device != positions.device:
            raise ValueError(f"lattices live on {lattices.device}, the positions on {positions.device}")
        if tuple(lattices.shape) != (positions.shape[0], 3, 3):
            raise ValueError(f"lattices has wrong shape: {tuple(lattices.shape)} != ({positions.shape[0]},3,3)")
        return lattices

    def calc_polarizabilities(self, positions_batch: NDArray[np.float64], dtype=None,
                              progress: bool = False, lattices=None) -> NDArray[np.float64]:
        """Polarizabilities ``(S,3,3)`` for fractional positions ``(S,N,3)``
        (``_gnn.py:667-721``): host arrays in, host arrays out.

        ``lattices`` (an addition; ``None`` = the reference structure's cell for every frame, the reference's behaviour):
        ``(S,3,3)``, one lattice per frame, rows = lattice vectors in Angstrom -- a variable-cell trajectory
        (``rn_potgnn_calc_polarizabilities_cells``).  Frame ``s`` is evaluated in ``lattices[s]`` as ``forward`` evaluates
        a sample in its lattice; the graph topology stays the reference structure's.  A non-finite or singular lattice
        raises ``ValueError`` naming the frame.

        ``progress=True`` shows the reference's progress bar (``tqdm``, unit " configs", ``_gnn.py:692,714-717``): the
        batch is then evaluated in blocks through the pipelined entry so that the bar moves; off by default -- one call
        is a fraction of a second for 10 000 frames.

        ``dtype`` is the arithmetic the model is evaluated in.  ``None`` follows
        ``torch.get_default_dtype()`` as the reference does (``_gnn.py:705-710``): float32 unless the
        caller ran ``torch.set_default_dtype(torch.float64)``; ``torch.float64`` / ``numpy.float64``
        selects the kernels instantiated for ``double`` (``rn_potgnn_calc_polarizabilities_f64``)."""
        pos = self._check_positions(positions_batch)
        lat = None if lattices is None else self._check_lattices(lattices, pos.shape[0])
        if self.training:  # as the reference does (_gnn.py:686); not walked again per call (the reference's unchanged
            self.eval()    # Phonons loop makes 2 M calls of one structure each, dynamics/_phonon.py:93-106)
        out = np.empty((pos.shape[0], 3, 3), dtype=np.float64)
        handle = self._ensure_handle()
        if lat is not None:
            cells = _lib.load().rn_potgnn_calc_polarizabilities_cells
            use_float64 = int(_wants_float64(dtype))
            block = pos.shape[0]
            if progress and pos.shape[0] > 0:
                from tqdm import tqdm
                block = max(1, min(pos.shape[0], 2000))
                progress_bar = tqdm(total=pos.shape[0], unit=" configs")
            try:
                for first in range(0, pos.shape[0], max(block, 1)):  # (each block with its own lattices)
                    n = min(block, pos.shape[0] - first)
                    rc = cells(handle, _ptr(pos[first:first + n]), _ptr(lat[first:first + n]), n, use_float64,
                               _ptr(out[first:first + n]))
                    _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities_cells")
                    if progress:
                        progress_bar.update(n)
            finally:
                if progress and pos.shape[0] > 0:
                    progress_bar.close()
            return out
        if progress and pos.shape[0] > 0:
            from tqdm import tqdm
            entry = (_lib.load().rn_potgnn_calc_polarizabilities_f64 if _wants_float64(dtype)
                     else _lib.load().rn_potgnn_calc_polarizabilities)
            block = max(1, min(pos.shape[0], 2000))
            with tqdm(total=pos.shape[0], unit=" configs") as progress_bar:
                for first in range(0, pos.shape[0], block):
                    n = min(block, pos.shape[0] - first)
                    rc = entry(handle, _ptr(pos[first:first + n]), n, _ptr(out[first:first + n]))
                    _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities")
                    progress_bar.update(n)
            return out
        if _wants_float64(dtype):
            rc = _lib.load().rn_potgnn_calc_polarizabilities_f64(handle, _ptr(pos), pos.shape[0], _ptr(out))
            _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities_f64")
            return out
        rc = _lib.load().rn_potgnn_calc_polarizabilities(handle, _ptr(pos), pos.shape[0], _ptr(out))
        _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities")
        return out

    @property
    def device_index(self) -> int:
        """HIP ordinal the model evaluates on."""
        if self._device is not None:
            return int(self._device)
        return torch.cuda.current_device() if torch.cuda.is_available() else 0

    def calc_polarizabilities_async(self, positions_batch: NDArray[np.float64],
                                    out: NDArray[np.float64]) -> None:
        """Pipelined form of ``calc_polarizabilities`` (``rn_potgnn_calc_polarizabilities_async``):
        enqueues copy-in, evaluation and copy-out and returns; ``out`` ``(S,3,3)`` is valid after
        ``wait()``.  ``positions_batch`` and ``out`` must be C-contiguous float64 arrays that stay
        alive and untouched until then (page-locked memory makes the copies asynchronous)."""
        verify_ndarray_shape("positions_batch", positions_batch, (None, self.num_atoms, 3))
        s = positions_batch.shape[0]
        for name, arr, shape in (("positions_batch", positions_batch, positions_batch.shape), ("out", out, (s, 3, 3))):
            if arr.dtype != np.float64 or not arr.flags.c_contiguous or tuple(arr.shape) != tuple(shape):
                raise ValueError(f"{name} must be a C-contiguous float64 array of shape {tuple(shape)}")
        self.eval()
        handle = self._ensure_handle()
        rc = _lib.load().rn_potgnn_calc_polarizabilities_async(handle, _ptr(positions_batch), s, _ptr(out))
        _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities_async")

    def wait(self) -> None:
        """Block until every ``calc_polarizabilities_async`` call has delivered its result."""
        if self._handle is not None:
            rc = _lib.load().rn_potgnn_wait(self._handle)
            _lib.check(rc, self._handle, "rn_potgnn_wait")

    def calc_polarizabilities_to_device(self, positions_batch: NDArray[np.float64],
                                        out: torch.Tensor | None = None, lattices=None) -> torch.Tensor:
        """``calc_polarizabilities`` with the result left in HBM (``rn_potgnn_calc_polarizabilities_to_device``): host
        ``float64[S,N,3]`` in, device ``float64[S,3,3]`` out, float32 arithmetic.  The upload is pipelined with the
        kernels (positions cast to float32 while staged: bit-identical results, half the PCIe bytes); torch's current
        stream is ordered behind the evaluation, so the tensor can go straight into a collective, and the evaluation
        behind what was queued on that stream before the call (an earlier reader of ``out``).  ``out``, when given, must
        be a contiguous ``float64[S,3,3]`` tensor on the model's device.  ``lattices``: host ``(S,3,3)``, one lattice per
        frame as in ``calc_polarizabilities`` (``rn_potgnn_calc_polarizabilities_cells_to_device``); they are staged and
        ordered like the positions."""
        pos = self._check_positions(positions_batch)
        lat = None if lattices is None else self._check_lattices(lattices, pos.shape[0])
        self.eval()
        device = torch.device("cuda", self.device_index)
        if out is None:
            out = torch.empty((pos.shape[0], 3, 3), dtype=torch.float64, device=device)
        else:
            _check_out(out, pos.shape[0], self.device_index)
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(device).cuda_stream
        if lat is not None:
            rc = _lib.load().rn_potgnn_calc_polarizabilities_cells_to_device(
                handle, _ptr(pos), _ptr(lat), pos.shape[0], C.c_void_p(out.data_ptr()), C.c_void_p(stream))
            _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities_cells_to_device")
            return out
        rc = _lib.load().rn_potgnn_calc_polarizabilities_to_device(handle, _ptr(pos), pos.shape[0],
                                                                   C.c_void_p(out.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_calc_polarizabilities_to_device")
        return out

    def calc_polarizabilities_device(self, positions: torch.Tensor, out: torch.Tensor | None = None,
                                     synchronize: bool = False, dtype=None, lattices=None) -> torch.Tensor:
        """Same computation on a device-resident ``float64[S,N,3]`` tensor; returns a device
        ``float64[S,3,3]`` tensor.  Work is enqueued on torch's current stream.  ``dtype`` is the
        arithmetic of the evaluation, resolved exactly as ``calc_polarizabilities`` does: ``None`` follows
        ``torch.get_default_dtype()`` (``_gnn.py:705-710``), ``torch.float64`` runs the kernels instantiated
        for ``double`` -- so the host, gloo and RCCL paths of ``ramannoodle_amd.parallel`` agree.  ``lattices``: a
        contiguous CUDA float64 ``(S,3,3)`` tensor, one lattice per frame (``rn_potgnn_forward_cells_device``); it must
        stay untouched until the work has finished, and its values are not inspected."""
        if not (positions.is_cuda and positions.dtype == torch.float64 and positions.is_contiguous()):
            raise ValueError("positions must be a contiguous float64 device tensor")
        if positions.dim() != 3 or tuple(positions.shape[1:]) != (self.num_atoms, 3):
            raise ValueError(f"positions_batch has wrong shape: {tuple(positions.shape)} != "
                             f"(_,{self.num_atoms},3)")
        s = positions.shape[0]
        if out is None:
            out = torch.empty((s, 3, 3), dtype=torch.float64, device=positions.device)
        else:
            _check_out(out, s, positions.device.index)
        if lattices is not None:
            lattices = self._check_device_lattices(lattices, positions)
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(positions.device).cuda_stream
        if lattices is not None:
            rc = _lib.load().rn_potgnn_forward_cells_device(
                handle, C.c_void_p(positions.data_ptr()), C.c_void_p(lattices.data_ptr()), s,
                int(_wants_float64(dtype)), C.c_void_p(out.data_ptr()), C.c_void_p(stream), int(synchronize))
            _lib.check(rc, handle, "rn_potgnn_forward_cells_device")
            return out
        if _wants_float64(dtype):
            rc = _lib.load().rn_potgnn_forward_device_f64(
                handle, C.c_void_p(positions.data_ptr()), s, C.c_void_p(out.data_ptr()), C.c_void_p(stream),
                int(synchronize))
            _lib.check(rc, handle, "rn_potgnn_forward_device_f64")
            return out
        rc = _lib.load().rn_potgnn_forward_device(
            handle, C.c_void_p(positions.data_ptr()), s, C.c_void_p(out.data_ptr()), None,
            C.c_void_p(stream), int(synchronize))
        _lib.check(rc, handle, "rn_potgnn_forward_device")
        return out

    @property
    def num_descriptor_columns(self) -> int:
        """The columns of a structure descriptor: the size of the edge embedding."""
        return int(self._fe)

    def calc_descriptors(self, positions_batch, lattices=None, float64: bool = False, with_polarizabilities: bool = False):
        """Structure descriptors ``(S, num_descriptor_columns)`` float64 of fractional positions ``(S,N,3)`` (an addition;
        ``rn_potgnn_descriptors``): per frame the mean over the edges of the edge embedding after the last message pass,
        the rows the readout turns into the polarizability -- the model's own latent space, for
        ``ramannoodle_amd.selection``.  ``lattices`` as for ``calc_polarizabilities``; ``float64`` runs the kernels
        instantiated for ``double``.  With ``with_polarizabilities`` the result is ``(descriptors, polarizabilities
        (S,3,3))`` from one evaluation, the polarizabilities bit for bit those of ``calc_polarizabilities``."""
        pos = self._check_positions(positions_batch)
        lat = None if lattices is None else self._check_lattices(lattices, pos.shape[0])
        if self.training:
            self.eval()
        desc = np.empty((pos.shape[0], self.num_descriptor_columns), dtype=np.float64)
        alpha = np.empty((pos.shape[0], 3, 3), dtype=np.float64) if with_polarizabilities else None
        handle = self._ensure_handle()
        rc = _lib.load().rn_potgnn_descriptors(handle, _ptr(pos), None if lat is None else _ptr(lat), pos.shape[0],
                                               int(bool(float64)), _ptr(desc), None if alpha is None else _ptr(alpha))
        _lib.check(rc, handle, "rn_potgnn_descriptors")
        return (desc, alpha) if with_polarizabilities else desc

    def calc_descriptors_device(self, positions: torch.Tensor, lattices=None, out: torch.Tensor | None = None,
                                alpha_out: torch.Tensor | None = None, float64: bool = False) -> torch.Tensor:
        """``calc_descriptors`` on a device-resident ``float64[S,N,3]`` tensor (``rn_potgnn_device_descriptors``):
        returns a device ``float64[S, num_descriptor_columns]`` tensor (``out``, when given).  ``alpha_out``, a contiguous
        ``float64[S,3,3]`` tensor on the same device, receives the polarizabilities of the same evaluation.  Work is
        enqueued on torch's current stream; ``lattices`` as for ``calc_polarizabilities_device``."""
        if not (positions.is_cuda and positions.dtype == torch.float64 and positions.is_contiguous()):
            raise ValueError("positions must be a contiguous float64 device tensor")
        if positions.dim() != 3 or tuple(positions.shape[1:]) != (self.num_atoms, 3):
            raise ValueError(f"positions_batch has wrong shape: {tuple(positions.shape)} != "
                             f"(_,{self.num_atoms},3)")
        s, columns = positions.shape[0], self.num_descriptor_columns
        if out is None:
            out = torch.empty((s, columns), dtype=torch.float64, device=positions.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
                  and tuple(out.shape) == (s, columns) and out.device == positions.device):
            raise ValueError(f"out must be a contiguous float64[{s},{columns}] tensor on {positions.device}")
        if alpha_out is not None:
            _check_out(alpha_out, s, positions.device.index)
        if lattices is not None:
            lattices = self._check_device_lattices(lattices, positions)
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(positions.device).cuda_stream
        rc = _lib.load().rn_potgnn_device_descriptors(
            handle, C.c_void_p(positions.data_ptr()), C.c_void_p(None if lattices is None else lattices.data_ptr()), s,
            int(bool(float64)), C.c_void_p(out.data_ptr()), C.c_void_p(None if alpha_out is None else alpha_out.data_ptr()),
            C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_device_descriptors")
        return out

    def forward(self, lattice, atomic_numbers, positions) -> torch.Tensor:
        """Standardised 6-vectors ``[S,6]`` (``_gnn.py:617-665``).  ``lattice`` ``[S,3,3]`` is
        used per sample in the geometry, as the reference does (``_gnn.py:603-611``), and
        ``atomic_numbers`` ``[S,N]`` per sample for the node embedding
        (``_convert_to_atom_type``, ``_gnn.py:541-557,642-643``), in evaluation AND in training mode; the graph
        topology is the reference structure's.  An atomic number the model has no atom type for raises
        ``IndexError``, as the reference's ``Embedding`` does.

        Arithmetic: the reference's ``forward`` computes in the dtype of the model's parameters (``_gnn.py:493-494``):
        float32 unless the caller ran ``torch.set_default_dtype(torch.float64)`` before constructing the model.  So does this
        one in EVALUATION mode: a model whose parameters are float64 (built under that default, or ``model.double()``) runs
        the kernels instantiated for ``double`` (``rn_potgnn_forward_samples_f64``) and returns a float64 tensor; the device
        keeps float32 master weights, so float64 parameters take part rounded to float32 (exact for a state dict that was
        trained in float32).  In TRAINING mode ``forward`` evaluates in float32 whatever the parameters' dtype (the float64
        step is ``train_gradients_f64``).  ``calc_polarizabilities(..., dtype=...)`` follows the default dtype when
        ``dtype`` is ``None`` (``_gnn.py:705-710``), as does ``calc_polarizabilities_device``.
        An evaluation-mode ``forward`` (or any other evaluation) between a training-mode ``forward`` and its ``backward()``
        reuses the device workspace the pending step's tape refers to: run ``backward()`` first -- the backward of a step
        whose tape was overwritten raises ``ValueError`` ("needs a preceding train_forward").

        The result lives where the inputs live, as the reference's does (``_train.py:51-75`` moves a batch to the
        device and takes the loss there; ``test/tests/torch/test_gnn.py:130-160``): CUDA tensors are evaluated in
        place in HBM (``rn_potgnn_forward_samples_device``: no copy through the host) and a CUDA tensor comes back;
        host tensors / arrays give a host tensor.

        Input gradients: with grad mode on and ``positions`` and / or ``lattice`` requiring grad, the result's backward
        fills ``positions.grad`` ``[S,N,3]`` (with respect to the FRACTIONAL positions, as ``alpha_jacobian``) and
        ``lattice.grad`` ``[S,3,3]`` (row i = lattice vector i; a lattice given as ``L.expand(S,3,3)`` gets the sum through
        torch's expand), in the dtype and on the device of each input (CUDA inputs: the work is ordered on torch's current
        stream at backward time; host inputs: host gradients).  ``atomic_numbers`` gets none.  Double backward raises
        ``RuntimeError``.
        * EVALUATION mode: the forward value is the one computed without gradients, bit for bit; ``backward`` recomputes
          the forward with its tape, a work chunk at a time (bounded memory for any S), and runs one reverse pass with
          one cotangent per frame (``rn_potgnn_forward_vjp_device``), in the dtype of the parameters (float32 kernels, or
          those instantiated for ``double`` for a float64 model).  The taped forward runs on different kernels from the
          fast evaluation, so a float32 gradient is that of the same function up to float32 rounding.  Like any
          evaluation, the backward reuses the device workspace and tape of lane 0: a training step whose forward ran
          before it and whose backward has not yet run raises ``ValueError`` afterwards.
        * TRAINING mode: the step's own reverse pass (batch-statistics BatchNorm, so one sample's gradient depends on the
          whole batch) writes the input gradients too (``rn_potgnn_train_backward_inputs(_device)``); the parameter
          gradients are bit-identical to those of a step whose inputs require no grad.
        With no input requiring grad, or under ``torch.no_grad()``, nothing of this runs: same entries, same bits, no
        tape."""
        if not self.training and torch.is_grad_enabled() and (_requires_grad(positions) or _requires_grad(lattice)):
            return _EvalInputGrad.apply(self, lattice, atomic_numbers, positions)
        pos_t, lat_t, zs_t = torch.as_tensor(positions), torch.as_tensor(lattice), torch.as_tensor(atomic_numbers)
        s = pos_t.shape[0] if pos_t.dim() == 3 else -1
        if pos_t.dim() != 3 or tuple(pos_t.shape[1:]) != (self.num_atoms, 3):
            verify_ndarray_shape("positions", pos_t.detach().cpu().numpy(), (None, self.num_atoms, 3))
        if tuple(lat_t.shape) != (s, 3, 3) or tuple(zs_t.shape) != (s, self.num_atoms):
            raise ValueError("lattice / atomic_numbers do not match positions")
        on_device = pos_t.is_cuda or lat_t.is_cuda or zs_t.is_cuda
        model_f64 = (not self.training) and next(self.parameters()).dtype == torch.float64
        if on_device and not self.training and not model_f64:
            return self._forward_on_device(lat_t, zs_t, pos_t)
        if on_device and self._device_training and getattr(self, "_dp_group", None) is None:
            # device-resident training on a device-resident batch: nothing crosses PCIe in either direction
            return _TrainStepOnDevice.apply(self, lat_t, zs_t, pos_t, self._device_anchor)
        out_device = next((t.device for t in (pos_t, lat_t, zs_t) if t.is_cuda), None)
        pos = np.ascontiguousarray(pos_t.detach().cpu().numpy(), dtype=np.float64)
        lat = np.ascontiguousarray(lat_t.detach().cpu().numpy(), dtype=np.float64)
        zs = zs_t.detach().cpu().numpy()
        same_species = (not s) or np.array_equal(zs, np.broadcast_to(
            np.asarray(self._ref_structure.atomic_numbers), zs.shape))
        same_lattice = (not s) or np.allclose(lat, self._ref_structure.lattice[None], rtol=1e-6, atol=1e-9)
        types = None
        if not same_species:
            zi = zs.astype(np.int64)
            if zi.min() < -self._atom_type_map.size or zi.max() >= self._atom_type_map.size:
                raise IndexError("atomic number outside the atom type map")
            types = np.ascontiguousarray(self._atom_type_map[zi], dtype=np.int32)
            if types.min() < 0:
                raise IndexError("index out of range in self: atomic_numbers holds a species the "
                                 "model has no atom type for")
        if self.training:
            extra = (None if same_lattice else lat, types)
            if self._device_training:  # parameter gradients stay in HBM: nothing for autograd to route but the inputs'
                out = _TrainStep.apply(self, pos, extra, pos_t, lat_t, self._device_anchor)
            else:
                out = _TrainStep.apply(self, pos, extra, pos_t, lat_t, *self.parameters())
            return out.to(out_device) if out_device is not None else out
        handle = self._ensure_handle()
        if model_f64:  # the model's parameters are float64: evaluate in double, as the reference does
            out64 = np.empty((s, 6), dtype=np.float64)
            rc = _lib.load().rn_potgnn_forward_samples_f64(
                handle, None if same_lattice else _ptr(lat), None if types is None else _ptr(types), _ptr(pos), s, _ptr(out64))
            _lib.check(rc, handle, "rn_potgnn_forward_samples_f64")
            result = torch.from_numpy(out64)
            return result.to(out_device) if out_device is not None else result
        out = np.empty((s, 6), dtype=np.float32)
        if same_lattice and same_species:
            rc = _lib.load().rn_potgnn_forward(handle, _ptr(pos), s, _ptr(out))
            _lib.check(rc, handle, "rn_potgnn_forward")
        else:
            rc = _lib.load().rn_potgnn_forward_samples(
                handle, None if same_lattice else _ptr(lat), None if types is None else _ptr(types),
                _ptr(pos), s, _ptr(out))
            _lib.check(rc, handle, "rn_potgnn_forward_samples")
        return torch.from_numpy(out)

    def _device_inputs(self, lat_t: torch.Tensor, zs_t: torch.Tensor, pos_t: torch.Tensor):
        """What the device entries take, from tensors of which at least one is on a GPU: every check and conversion is a
        torch operation on the device.  Returns ``(device, S, positions f64 [S,N,3], lattices f32 [S,9] or None, atom types
        int32 [S,N] or None)``."""
        device = next(t.device for t in (pos_t, lat_t, zs_t) if t.is_cuda)
        if device.index is not None and self._device is not None and device.index != int(self._device):
            raise ValueError(f"inputs live on {device}, the model evaluates on cuda:{int(self._device)}")
        s = pos_t.shape[0]
        pos = pos_t.detach().to(device=device, dtype=torch.float64).contiguous()
        lat = lat_t.detach().to(device=device, dtype=torch.float64)
        zs = zs_t.detach().to(device=device)
        if s == 0:
            return device, s, pos, None, None
        ref_lat = torch.as_tensor(np.asarray(self._ref_structure.lattice, dtype=np.float64), device=device)
        ref_zs = torch.as_tensor(np.asarray(self._ref_structure.atomic_numbers), device=device).to(zs.dtype)
        same_lattice = bool(torch.allclose(lat, ref_lat.expand_as(lat), rtol=1e-6, atol=1e-9))
        same_species = bool(torch.equal(zs, ref_zs.expand_as(zs)))
        lat32 = types = None
        if not same_lattice:
            lat32 = lat.to(torch.float32).reshape(s, 9).contiguous()  # the reference's forward computes in float32
        if not same_species:
            zi = zs.to(torch.int64)
            size = self._atom_type_map.size
            if int(zi.min()) < -size or int(zi.max()) >= size:
                raise IndexError("atomic number outside the atom type map")
            tmap = torch.as_tensor(np.asarray(self._atom_type_map, dtype=np.int32), device=device)
            types = tmap[zi].contiguous()  # (negative atomic numbers index from the end, as numpy does on the host path)
            if int(types.min()) < 0:
                raise IndexError("index out of range in self: atomic_numbers holds a species the "
                                 "model has no atom type for")
        return device, s, pos, lat32, types

    def _forward_on_device(self, lat_t: torch.Tensor, zs_t: torch.Tensor, pos_t: torch.Tensor) -> torch.Tensor:
        """Evaluation-mode ``forward`` on device-resident inputs: the kernels read the tensors where they are, the ``[S,6]``
        result is a device tensor."""
        device, s, pos, lat32, types = self._device_inputs(lat_t, zs_t, pos_t)
        out = torch.empty((s, 6), dtype=torch.float32, device=device)
        if s == 0:
            return out
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = _lib.load().rn_potgnn_forward_samples_device(
            handle, None if lat32 is None else C.c_void_p(lat32.data_ptr()),
            None if types is None else C.c_void_p(types.data_ptr()), C.c_void_p(pos.data_ptr()), s,
            C.c_void_p(out.data_ptr()), C.c_void_p(stream), 1)
        _lib.check(rc, handle, "rn_potgnn_forward_samples_device")
        return out

    def _train_forward_on_device(self, lat_t: torch.Tensor, zs_t: torch.Tensor, pos_t: torch.Tensor) -> torch.Tensor:
        """Training-mode ``forward`` of a device-resident batch with device-resident weights
        (``rn_potgnn_train_forward_samples_device``): enqueued behind torch's current stream, no synchronisation."""
        device, s, pos, lat32, types = self._device_inputs(lat_t, zs_t, pos_t)
        if s == 0:
            raise ValueError("a training batch needs at least one structure")
        out = torch.empty((s, 6), dtype=torch.float32, device=device)
        handle = self._ensure_handle()
        self._install_reducer(handle)  # (no data-parallel group here: clears one that was installed before)
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = _lib.load().rn_potgnn_train_forward_samples_device(
            handle, None if lat32 is None else C.c_void_p(lat32.data_ptr()),
            None if types is None else C.c_void_p(types.data_ptr()), C.c_void_p(pos.data_ptr()), s,
            C.c_void_p(out.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_train_forward_samples_device")
        self._device_batches_tracked += 1  # (the library updated the running statistics where they live)
        self._device_ahead = True
        return out

    def _train_backward_on_device(self, grad_out: torch.Tensor, want_pos: bool = False, want_lat: bool = False):
        """Reverse pass of the pending device-resident step; with ``want_pos`` / ``want_lat`` the same pass also writes the
        input gradients, returned as device float64 ``([S,N,3] or None, [S,9] or None)``."""
        dvec6 = grad_out.detach().to(dtype=torch.float32).contiguous()
        stream = torch.cuda.current_stream(dvec6.device).cuda_stream
        if not (want_pos or want_lat):
            rc = _lib.load().rn_potgnn_train_backward_samples_device(self._handle, C.c_void_p(dvec6.data_ptr()),
                                                                     C.c_void_p(stream))
            _lib.check(rc, self._handle, "rn_potgnn_train_backward_samples_device")
            return None, None
        s = dvec6.shape[0]
        dpos = torch.empty((s, self.num_atoms, 3), dtype=torch.float64, device=dvec6.device) if want_pos else None
        dlat = torch.empty((s, 9), dtype=torch.float64, device=dvec6.device) if want_lat else None
        rc = _lib.load().rn_potgnn_train_backward_inputs_device(
            self._handle, C.c_void_p(dvec6.data_ptr()), None if dpos is None else C.c_void_p(dpos.data_ptr()),
            None if dlat is None else C.c_void_p(dlat.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, self._handle, "rn_potgnn_train_backward_inputs_device")
        return dpos, dlat

    def _input_gradients(self, lat_t: torch.Tensor, zs, pos_t: torch.Tensor, grad_out: torch.Tensor, want_pos: bool,
                         want_lat: bool):
        """Evaluation-mode input gradients (``rn_potgnn_forward_vjp_device``): device float64 ``([S,N,3] or None,
        [S,9] or None)`` on the inputs' GPU (the model's for host inputs), ordered on torch's current stream there."""
        zs_t = torch.as_tensor(zs)
        home = next((t.device for t in (pos_t, lat_t, zs_t) if t.is_cuda), None)
        device = home if home is not None else torch.device("cuda", self.device_index)
        device, s, pos, _, types = self._device_inputs(lat_t.detach().to(device), zs_t.to(device), pos_t.detach().to(device))
        dpos = torch.zeros((s, self.num_atoms, 3), dtype=torch.float64, device=device) if want_pos else None
        dlat = torch.zeros((s, 9), dtype=torch.float64, device=device) if want_lat else None
        if s == 0 or not (want_pos or want_lat):
            return dpos, dlat
        lat64 = lat_t.detach().to(device=device, dtype=torch.float64).reshape(s, 9).contiguous()
        dvec6 = grad_out.detach().to(device=device, dtype=torch.float64).contiguous()
        model_f64 = next(self.parameters()).dtype == torch.float64  # the precision forward evaluated in
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = _lib.load().rn_potgnn_forward_vjp_device(
            handle, C.c_void_p(lat64.data_ptr()), None if types is None else C.c_void_p(types.data_ptr()),
            C.c_void_p(pos.data_ptr()), s, C.c_void_p(dvec6.data_ptr()), int(model_f64),
            None if dpos is None else C.c_void_p(dpos.data_ptr()), None if dlat is None else C.c_void_p(dlat.data_ptr()),
            C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_forward_vjp_device")
        return dpos, dlat

    # -- training step pieces used by _TrainStep ------------------------------------------
    def enable_data_parallel(self, group=None) -> None:
        """Data-parallel training over the ranks of ``group`` (default process group): the
        readout BatchNorm then uses the statistics of the global batch (all-reduced column
        sums inside the device step, ``rn_potgnn_set_stat_reducer``); gradient averaging is
        ``ramannoodle_amd.parallel.average_gradients`` (``train_single_epoch`` calls it).
        ``None`` world / single rank: no effect."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            self._dp_group, self._dp_callback = None, None
        else:
            on_gpu = dist.get_backend(group) == "nccl"

            def _sum_over_ranks(values, count, _ctx):
                try:
                    view = np.ctypeslib.as_array(values, shape=(count,))
                    tensor = torch.from_numpy(view.copy())
                    if on_gpu:
                        tensor = tensor.cuda()
                    dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=group)
                    view[:] = tensor.cpu().numpy()
                    return 0
                except Exception:  # pylint: disable=broad-except  (must not unwind through C)
                    return 1

            self._dp_group = group if group is not None else dist.group.WORLD
            self._dp_callback = _REDUCE_FN(_sum_over_ranks)  # keep the thunk alive
        self._dp_installed_on = None

    @property
    def data_parallel_group(self):
        """Process group set by ``enable_data_parallel`` (``None`` = single process)."""
        return getattr(self, "_dp_group", None)

    def _install_reducer(self, handle) -> None:
        callback = getattr(self, "_dp_callback", None)
        if getattr(self, "_dp_installed_on", None) == (handle, id(callback)):
            return
        rc = _lib.load().rn_potgnn_set_stat_reducer(handle, C.cast(callback, C.c_void_p) if callback else None,
                                                    None)
        _lib.check(rc, handle, "rn_potgnn_set_stat_reducer")
        self._dp_installed_on = (handle, id(callback))

    def _train_forward(self, pos: np.ndarray, lat: np.ndarray | None = None, types: np.ndarray | None = None) -> np.ndarray:
        handle = self._ensure_handle()
        self._install_reducer(handle)
        out = np.empty((pos.shape[0], 6), dtype=np.float32)
        mean = np.empty(self._fe, dtype=np.float32)
        var = np.empty(self._fe, dtype=np.float32)
        if lat is None and types is None:
            rc = _lib.load().rn_potgnn_train_forward(handle, _ptr(pos), pos.shape[0], _ptr(out),
                                                     _ptr(mean), _ptr(var))
            _lib.check(rc, handle, "rn_potgnn_train_forward")
        else:  # a lattice and / or atom types per sample (_gnn.py:603-611, 541-557)
            rc = _lib.load().rn_potgnn_train_forward_samples(
                handle, None if lat is None else _ptr(lat), None if types is None else _ptr(types), _ptr(pos),
                pos.shape[0], _ptr(out), _ptr(mean), _ptr(var))
            _lib.check(rc, handle, "rn_potgnn_train_forward_samples")
        if self._device_training:  # the library updated the running statistics where they live
            self._device_batches_tracked += 1
            self._device_ahead = True
            return out
        # BatchNorm1d running statistics, torch semantics (momentum 0.1, unbiased variance)
        rows = int(round(_lib.load().rn_potgnn_train_row_count(handle)))  # all ranks' rows
        pre = "_to_polarizability_embedding.1."
        with torch.no_grad():
            running_mean, running_var = self._state[pre + "running_mean"], self._state[pre + "running_var"]
            running_mean.mul_(0.9).add_(torch.from_numpy(mean).to(running_mean.device) * 0.1)
            unbiased = torch.from_numpy(var).to(running_var.device) * (rows / max(rows - 1, 1))
            running_var.mul_(0.9).add_(unbiased * 0.1)
            self._state[pre + "num_batches_tracked"].add_(1)
        self._uploaded_version = None  # buffers changed: re-upload before the next evaluation
        return out

    def _train_backward(self, dvec6: np.ndarray, dpos: np.ndarray | None = None, dlat: np.ndarray | None = None):
        handle = self._handle
        lib = _lib.load()
        blob = np.empty(sum(v.numel() for v in self._state.values() if v.is_floating_point()),
                        dtype=np.float32)
        if dpos is None and dlat is None:
            rc = lib.rn_potgnn_train_backward(handle, _ptr(dvec6), _ptr(blob))
            _lib.check(rc, handle, "rn_potgnn_train_backward")
        else:  # the same reverse pass, writing the input gradients too
            rc = lib.rn_potgnn_train_backward_inputs(handle, _ptr(dvec6), _ptr(blob), None if dpos is None else _ptr(dpos),
                                                     None if dlat is None else _ptr(dlat))
            _lib.check(rc, handle, "rn_potgnn_train_backward_inputs")
        grads, offset = [], 0
        for key, value in self._state.items():
            if not value.is_floating_point():
                continue
            n = value.numel()
            if self._is_trainable(key):
                grads.append(torch.from_numpy(blob[offset:offset + n].reshape(tuple(value.shape)).copy()))
            offset += n
        return grads

    # -- device-resident optimisation (DeviceAdam) ------------------------------------------
    def enable_device_training(self, enabled: bool = True) -> None:
        """Keep parameter gradients, optimiser state and BatchNorm running statistics in HBM
        (``rn_potgnn_train_backward_device`` / ``rn_potgnn_adam_step``): a training step then
        moves only positions, outputs and ``dL/dout`` across PCIe.  ``parameters()`` /
        ``state_dict()`` fetch the current values on demand; ``p.grad`` is not populated."""
        handle = self._ensure_handle()
        if not enabled:
            _ = self._state  # bring the host copy up to date before handing control back
        rc = _lib.load().rn_potgnn_set_device_training(handle, int(bool(enabled)))
        _lib.check(rc, handle, "rn_potgnn_set_device_training")
        self._device_training = bool(enabled)
        self._device_batches_tracked = int(
            self._state_store["_to_polarizability_embedding.1.num_batches_tracked"])

    def _train_backward_device(self, dvec6: np.ndarray, dpos: np.ndarray | None = None,
                               dlat: np.ndarray | None = None) -> None:
        if dpos is None and dlat is None:
            rc = _lib.load().rn_potgnn_train_backward_device(self._handle, _ptr(dvec6))
            _lib.check(rc, self._handle, "rn_potgnn_train_backward_device")
            return
        rc = _lib.load().rn_potgnn_train_backward_inputs(self._handle, _ptr(dvec6), None,
                                                         None if dpos is None else _ptr(dpos),
                                                         None if dlat is None else _ptr(dlat))
        _lib.check(rc, self._handle, "rn_potgnn_train_backward_inputs")

    def device_gradients(self) -> torch.Tensor:
        """The float32 gradient buffer of the last device backward, as a CUDA tensor that
        aliases the library's memory (packed layout; for in-place all-reduce over RCCL)."""
        ptr, count = C.c_void_p(), C.c_size_t()
        rc = _lib.load().rn_potgnn_gradient_buffer(self._handle, C.byref(ptr), C.byref(count))
        _lib.check(rc, self._handle, "rn_potgnn_gradient_buffer")
        return _alias_device_buffer(int(ptr.value), int(count.value), self.device_index)

    def _adam_step(self, lr, beta1, beta2, eps, weight_decay, step) -> None:
        rc = _lib.load().rn_potgnn_adam_step(self._handle, lr, beta1, beta2, eps, weight_decay, step)
        _lib.check(rc, self._handle, "rn_potgnn_adam_step")
        self._device_ahead = True

    def train_gradients_f64(self, positions, targets, lattice=None, atomic_numbers=None):
        """One training step's forward and backward in float64 on the device
        (``rn_potgnn_train_forward_f64`` / ``_backward_f64``) for an MSE loss against ``targets``
        ``[S,6]``: returns ``(out [S,6] float64, loss, {parameter name: gradient float64})``.
        ``lattice`` ``[S,3,3]`` / ``atomic_numbers`` ``[S,N]``: per-sample inputs as ``forward`` takes them.
        Validation aid: what the float32 step is measured against; running statistics are not
        updated."""
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        verify_ndarray_shape("positions", pos, (None, self.num_atoms, 3))
        tgt = np.ascontiguousarray(targets, dtype=np.float64)
        s = pos.shape[0]
        handle = self._ensure_handle()
        self._install_reducer(handle)
        lib = _lib.load()
        out = np.empty((s, 6), dtype=np.float64)
        mean, var = np.empty(self._fe), np.empty(self._fe)
        lat = None if lattice is None else np.ascontiguousarray(lattice, dtype=np.float64).reshape(s, 3, 3)
        types = None
        if atomic_numbers is not None:
            types = np.ascontiguousarray(self._atom_type_map[np.asarray(atomic_numbers, dtype=np.int64)], dtype=np.int32)
        if lat is None and types is None:
            rc = lib.rn_potgnn_train_forward_f64(handle, _ptr(pos), s, _ptr(out), _ptr(mean), _ptr(var))
            _lib.check(rc, handle, "rn_potgnn_train_forward_f64")
        else:
            rc = lib.rn_potgnn_train_forward_samples_f64(handle, None if lat is None else _ptr(lat),
                                                         None if types is None else _ptr(types), _ptr(pos), s, _ptr(out),
                                                         _ptr(mean), _ptr(var))
            _lib.check(rc, handle, "rn_potgnn_train_forward_samples_f64")
        loss = float(np.mean((out - tgt) ** 2))
        dvec6 = np.ascontiguousarray(2.0 * (out - tgt) / out.size)
        blob = np.empty(sum(v.numel() for v in self._state.values() if v.is_floating_point()), dtype=np.float64)
        rc = lib.rn_potgnn_train_backward_f64(handle, _ptr(dvec6), _ptr(blob))
        _lib.check(rc, handle, "rn_potgnn_train_backward_f64")
        grads, offset = {}, 0
        for key, value in self._state.items():
            if not value.is_floating_point():
                continue
            n = value.numel()
            if self._is_trainable(key):
                grads[key] = blob[offset:offset + n].reshape(tuple(value.shape)).copy()
            offset += n
        return out, loss, grads

    def calc_raman_tensors(self, ref_positions, displacements,
                           delta: float = RAMAN_TENSOR_CENTRAL_DIFFERENCE,
                           method: str = "finite-difference") -> NDArray[np.float64]:
        """Raman tensors of all modes in one device call.

        ``method="finite-difference"`` (default, the reference's definition):
        ``(alpha(r + delta d_m) - alpha(r - delta d_m)) / delta`` in one float64 batch of the
        ``2M`` displaced cells (``dynamics/_phonon.py:93-106``).
        ``method="analytic"``: ``2 (d alpha / d r) . d_m`` from one forward and one reverse
        pass (equal up to ``O(delta^2)``).
        """
        self._check_raman_arguments(ref_positions, displacements, delta=delta, method=method)
        ref = np.ascontiguousarray(ref_positions, dtype=np.float64)
        disp = np.ascontiguousarray(displacements, dtype=np.float64)
        out = np.empty((disp.shape[0], 3, 3), dtype=np.float64)
        handle = self._ensure_handle()
        lib = _lib.load()
        if method == "analytic":
            rc = lib.rn_potgnn_raman_tensors_analytic(handle, _ptr(ref), _ptr(disp), disp.shape[0],
                                                      _ptr(out))
            _lib.check(rc, handle, "rn_potgnn_raman_tensors_analytic")
        elif method == "finite-difference":
            rc = lib.rn_potgnn_raman_tensors(handle, _ptr(ref), _ptr(disp), disp.shape[0],
                                             float(delta), _ptr(out))
            _lib.check(rc, handle, "rn_potgnn_raman_tensors")
        else:
            raise ValueError(f"unsupported method: {method}")
        return out

    def _check_raman_arguments(self, ref_positions, displacements, delta: float = RAMAN_TENSOR_CENTRAL_DIFFERENCE,
                               method: str = "finite-difference", **unknown) -> None:
        """Argument checks of ``calc_raman_tensors`` (also run by ``parallel.calc_raman_tensors_sharded`` on every
        rank before it branches, so that all ranks raise together)."""
        if unknown:
            raise TypeError(f"calc_raman_tensors() got unexpected keyword arguments: {sorted(unknown)}")
        raman_arguments(ref_positions, displacements, delta, method, self.num_atoms)

    def alpha_jacobian(self, positions, float64: bool = True) -> NDArray[np.float64]:
        """``d vec6_k / d x_{n,c}`` of the standardised 6-vector at one structure,
        ``(6, N, 3)``, by reverse-mode differentiation on the device."""
        verify_ndarray_shape("positions", positions, (self.num_atoms, 3))
        pos = np.ascontiguousarray(positions, dtype=np.float64)
        out = np.empty((6, self.num_atoms, 3), dtype=np.float64)
        handle = self._ensure_handle()
        rc = _lib.load().rn_potgnn_alpha_jacobian(handle, _ptr(pos), int(float64), _ptr(out))
        _lib.check(rc, handle, "rn_potgnn_alpha_jacobian")
        return out

    # ------------------------------------------------------------------ atom-group decomposition
    _partial_raman_entry = "rn_potgnn_partial_raman_tensors"  # (what DeviceIncrements asks of a model)
    _check_status = staticmethod(_lib.check)

    def calc_group_increments_device(self, positions: torch.Tensor, groups, float64: bool = True,
                                     out: torch.Tensor | None = None, workspace_limit: int = 0,
                                     lattices=None) -> torch.Tensor:
        """Per-group trapezoid increments of the polarizability along a trajectory
        (``rn_potgnn_group_increments_device``): a contiguous float64 CUDA tensor ``(S,N,3)`` of fractional, wrapped
        positions in, a float64 CUDA tensor ``(S-1,G,3,3)`` out,
        ``out[t,g] = 1/2 sum_{i in g} (J_i(x_t) + J_i(x_{t+1})) . dx_{t,i}`` with ``J_i = d alpha / d x_i`` (evaluation
        mode, ``float64`` or float32 arithmetic) and ``dx`` the minimum image of ``x_{t+1} - x_t``.  ``sum_g out[t]`` is
        ``alpha(x_{t+1}) - alpha(x_t)`` up to the trapezoid error.  ``groups``: ``spectrum.group_labels``.  Ordered on
        torch's current stream.  ``out``, when given, must be a contiguous float64 ``(S-1,G,3,3)`` tensor on the
        positions' device.

        ``lattices`` (a contiguous CUDA float64 ``(S,3,3)`` tensor, one lattice per frame;
        ``rn_potgnn_group_increments_cells_device``): a variable cell.  Every ``J`` is then taken at its frame's own lattice
        and the result is ``(S-1,G+1,3,3)``: **the last group is the cell**,
        ``out[t,G] = 1/2 (J_L(t) + J_L(t+1)) : (L_{t+1} - L_t)`` with ``J_L = d alpha / d L``, the change of the
        polarizability because the cell deforms at fixed fractional positions.  The sum over all ``G+1`` channels is
        ``alpha(t+1) - alpha(t)`` up to the trapezoid error; without the cell channel it is not.  The cell counts as a
        group: more than 15 atom groups together with lattices raise ``ValueError``."""
        # (no device_index: the positions' device is not compared with the model's, here and for the modes)
        s = device_frames(positions, self.num_atoms, 2, "group increments")
        labels, num_groups = self._group_labels(groups)
        if lattices is not None:
            lattices = self._check_device_lattices(lattices, positions)
            from ramannoodle_amd.spectrum import MAX_GROUPS
            if num_groups + 1 > MAX_GROUPS:
                raise ValueError(f"{num_groups} atom groups and the cell are more than {MAX_GROUPS} channels: with lattices "
                                 f"at most {MAX_GROUPS - 1} atom groups")
        out = device_out(out, positions, (s - 1, num_groups + (lattices is not None), 3, 3))
        self.eval()
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(positions.device).cuda_stream
        if lattices is not None:
            rc = _lib.load().rn_potgnn_group_increments_cells_device(
                handle, C.c_void_p(positions.data_ptr()), C.c_void_p(lattices.data_ptr()), s, _ptr(labels), num_groups,
                int(float64), int(workspace_limit), C.c_void_p(out.data_ptr()), C.c_void_p(stream))
            _lib.check(rc, handle, "rn_potgnn_group_increments_cells_device")
            return out
        rc = _lib.load().rn_potgnn_group_increments_device(
            handle, C.c_void_p(positions.data_ptr()), s, _ptr(labels), num_groups, int(float64), int(workspace_limit),
            C.c_void_p(out.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_group_increments_device")
        return out

    def calc_group_increments(self, positions_ts, groups, float64: bool = True, lattices=None) -> NDArray[np.float64]:
        """``calc_group_increments_device`` for host arrays: fractional positions ``(S,N,3)`` in, float64
        ``(S-1,G,3,3)`` out.  ``lattices``: host ``(S,3,3)``, one lattice per frame; the result is then
        ``(S-1,G+1,3,3)`` and the last group is the cell.  Non-finite or singular lattices raise ``ValueError``."""
        return self._increments_from_host(self.calc_group_increments_device, positions_ts, lattices, groups,
                                          float64=float64)

    def calc_partial_raman_tensors(self, ref_positions, displacements, groups) -> NDArray[np.float64]:
        """Raman tensors split by atom group, ``(M,G,3,3)``: ``R[m,g] = 2 sum_{i in g} J_i(ref) . d_{m,i}``
        (``rn_potgnn_partial_raman_tensors``: one float64 Jacobian, then the device contraction), so that
        ``sum_g R[m,g]`` is ``calc_raman_tensors(method="analytic")``."""
        self._check_raman_arguments(ref_positions, displacements, method="analytic")
        self.eval()
        return self._partial_raman_tensors(ref_positions, displacements, groups)

    # ------------------------------------------------------------------ phonon-mode decomposition
    def calc_mode_increments_device(self, positions: torch.Tensor, displacements, projectors, rest: bool = True,
                                    float64: bool = True, out: torch.Tensor | None = None, workspace_limit: int = 0,
                                    lattices=None) -> torch.Tensor:
        """Per-mode trapezoid increments of the polarizability along a trajectory (``rn_potgnn_mode_increments_device``):
        ``calc_group_increments_device`` split by phonon mode instead of by atom group.  ``positions``: a contiguous
        float64 CUDA tensor ``(S,N,3)``; ``displacements`` and ``projectors``: the host arrays ``(D, P)`` of
        ``spectrum.mode_projectors``, ``(M,N,3)`` each, any ``M >= 1``.  Out: a float64 CUDA tensor ``(S-1,C,3,3)``,
        ``out[t,m] = (1/2 (J(x_t) + J(x_{t+1})) . D[m]) (P[m] . dx_t)`` for ``m < M``: the change of the polarizability
        along mode m times the step's amplitude in mode m, contracted on the float64 matrix pipe.  ``rest=True`` adds
        channel ``M``, the one-group increment minus the modes' sum (round-off for a complete set, the unselected modes
        otherwise); ``lattices`` (as for ``calc_group_increments_device``) adds the cell channel, the last.  The
        channels, ``[modes..., rest?, cell?]``, sum to what the atom groups sum to.  Ordered on torch's current stream;
        ``out`` as for ``calc_group_increments_device``."""
        s = device_frames(positions, self.num_atoms, 2, "mode increments")
        disp, proj = mode_arrays(displacements, projectors, self.num_atoms)
        if lattices is not None:
            lattices = self._check_device_lattices(lattices, positions)
        channels = disp.shape[0] + bool(rest) + (lattices is not None)
        out = device_out(out, positions, (s - 1, channels, 3, 3))
        self.eval()
        handle = self._ensure_handle()
        stream = torch.cuda.current_stream(positions.device).cuda_stream
        rc = _lib.load().rn_potgnn_mode_increments_device(
            handle, C.c_void_p(positions.data_ptr()), C.c_void_p(lattices.data_ptr() if lattices is not None else None),
            s, _ptr(disp), _ptr(proj), disp.shape[0], int(bool(rest)), int(float64), int(workspace_limit),
            C.c_void_p(out.data_ptr()), C.c_void_p(stream))
        _lib.check(rc, handle, "rn_potgnn_mode_increments_device")
        return out

    def calc_mode_increments(self, positions_ts, displacements, projectors, rest: bool = True, float64: bool = True,
                             lattices=None) -> NDArray[np.float64]:
        """``calc_mode_increments_device`` for host arrays: fractional positions ``(S,N,3)`` in, float64
        ``(S-1,C,3,3)`` out; ``lattices``: host ``(S,3,3)`` (non-finite or singular lattices raise ``ValueError``)."""
        return self._increments_from_host(self.calc_mode_increments_device, positions_ts, lattices, displacements,
                                          projectors, rest=rest, float64=float64)

    # ------------------------------------------------------------------ introspection
    @property
    def num_triplets(self) -> int:
        """Number of edge triplets (k->j, j->i, i != k) of the frozen graph."""
        return int(_lib.load().rn_potgnn_num_triplets(self._ensure_handle()))

    def triplets(self):
        """Edge triplets as the device enumerates them, re-sorted into the reference's
        order: ``(i, j, idx_i, idx_j, idx_k, slot5, slot6)`` int64 arrays with the meaning of
        ``BatchTriplets._ref_triplets`` (``_utils.py:161-168``)."""
        handle = self._ensure_handle()
        lib = _lib.load()
        t = int(lib.rn_potgnn_num_triplets(handle))
        arrs = [np.empty(t, dtype=np.int32) for _ in range(5)]
        rc = lib.rn_potgnn_debug_triplets(handle, *[_ptr(a) for a in arrs])
        _lib.check(rc, handle, "rn_potgnn_debug_triplets")
        idx_i, idx_j, idx_k, slot5, slot6 = [a.astype(np.int64) for a in arrs]
        order = np.lexsort((idx_k, slot6))  # by source edge (j->i), then k
        return (self._ref_edge_indexes[2].copy(), self._ref_edge_indexes[1].copy(),
                idx_i[order], idx_j[order], idx_k[order], slot5[order], slot6[order])

    def device_triplets_raw(self):
        """Triplets in device aggregation order (grouped by destination edge)."""
        handle = self._ensure_handle()
        lib = _lib.load()
        t = int(lib.rn_potgnn_num_triplets(handle))
        arrs = [np.empty(t, dtype=np.int32) for _ in range(5)]
        _lib.check(lib.rn_potgnn_debug_triplets(handle, *[_ptr(a) for a in arrs]), handle,
                   "rn_potgnn_debug_triplets")
        return arrs

    def debug_stage(self, stage: int, index: int = 0) -> np.ndarray:
        """Intermediate of the last evaluation's last chunk (see ``rn_potgnn.h``)."""
        handle = self._ensure_handle()
        lib = _lib.load()
        cap = 64 * 1024 * 1024
        buf = np.empty(cap, dtype=np.float32)
        rows, cols = C.c_int64(), C.c_int64()
        rc = lib.rn_potgnn_debug_stage(handle, stage, index, _ptr(buf), cap, C.byref(rows),
                                       C.byref(cols))
        _lib.check(rc, handle, "rn_potgnn_debug_stage")
        return buf[: rows.value * cols.value].reshape(rows.value, cols.value).copy()

    def config_flags(self) -> dict:
        """Which kernel variants the handle selected (``rn_potgnn_config_flags``)."""
        flags = _lib.load().rn_potgnn_config_flags(self._ensure_handle())
        return {"fused_edge_block": bool(flags & 1), "folded_gate_scale": bool(flags & 2),
                "split_f16_mfma": bool(flags & 4), "narrow_kernels": bool(flags & 8),
                "mfma_range_fallback": bool(flags & 16),
                "role_split_edge_block": bool(flags & 256), "atom_owning_node_block": bool(flags & 512),
                "split_f16_pair_rows": bool(flags & 1024), "c2_per_atom_pair": bool(flags & 2048)}

    def set_profiling(self, mode: int) -> None:
        """0 = off, 1 = HIP-event timing of every kernel launch, 100+k = kernel k only."""
        self._profiling = int(mode)
        if self._handle is not None:
            _lib.load().rn_potgnn_set_profiling(self._handle, self._profiling)

    def kernel_times(self) -> dict:
        """``{kernel: (milliseconds, launches)}`` accumulated since ``set_profiling``."""
        handle = self._ensure_handle()
        lib = _lib.load()
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        launches = (C.c_int64 * 16)()
        n = lib.rn_potgnn_kernel_times(handle, names, ms, launches, 16)
        return {names[i].decode(): (ms[i], launches[i]) for i in range(max(n, 0))}


def _requires_grad(value) -> bool:
    return isinstance(value, torch.Tensor) and value.requires_grad


def _as_input_grad(grad, like: torch.Tensor):
    """A float64 gradient in the shape, dtype and on the device of the input it belongs to."""
    if grad is None:
        return None
    return grad.reshape(like.shape).to(device=like.device, dtype=like.dtype)


class _EvalInputGrad(torch.autograd.Function):
    """``PotGNN.forward`` in evaluation mode with positions and / or lattice requiring grad: the value is the plain
    evaluation's (``forward`` under no grad), the backward is ``rn_potgnn_forward_vjp_device``."""

    @staticmethod
    def forward(ctx, model, lattice, atomic_numbers, positions):  # pylint: disable=arguments-differ
        ctx.model = model
        ctx.atomic_numbers = atomic_numbers
        # (the inputs themselves: their gradients go back in their dtype, on their device)
        lat_t = lattice if isinstance(lattice, torch.Tensor) else torch.as_tensor(lattice)
        pos_t = positions if isinstance(positions, torch.Tensor) else torch.as_tensor(positions)
        ctx.save_for_backward(lat_t, pos_t)
        return model.forward(lattice, atomic_numbers, positions)  # (grad mode is off in here: the plain path)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # pylint: disable=arguments-differ
        lat_t, pos_t = ctx.saved_tensors
        want_lat, want_pos = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        dpos, dlat = ctx.model._input_gradients(lat_t, ctx.atomic_numbers, pos_t, grad_out, want_pos, want_lat)
        return (None, _as_input_grad(dlat, lat_t) if want_lat else None, None,
                _as_input_grad(dpos, pos_t) if want_pos else None)


class _TrainStep(torch.autograd.Function):
    """``PotGNN.forward`` in training mode: forward and backward both run on the device
    (``rn_potgnn_train_forward`` / ``rn_potgnn_train_backward``); autograd only routes the
    parameter gradients and, when the position / lattice tensors ``pos_t`` / ``lat_t`` require grad, theirs
    (``rn_potgnn_train_backward_inputs``: the same reverse pass)."""

    @staticmethod
    def forward(ctx, model, pos, extra, pos_t, lat_t, *params):  # pylint: disable=arguments-differ
        ctx.model = model
        ctx.inputs = (pos_t.detach(), lat_t.detach())  # (shape, dtype and device of their gradients)
        return torch.from_numpy(model._train_forward(pos, *extra))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # pylint: disable=arguments-differ
        dvec6 = np.ascontiguousarray(grad_out.detach().cpu().numpy(), dtype=np.float32)
        want_pos, want_lat = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        s = dvec6.shape[0]
        dpos = np.empty((s, ctx.model.num_atoms, 3), dtype=np.float64) if want_pos else None
        dlat = np.empty((s, 9), dtype=np.float64) if want_lat else None
        if ctx.model._device_training:
            ctx.model._train_backward_device(dvec6, dpos, dlat)
            params = []
        else:
            grads = ctx.model._train_backward(dvec6, dpos, dlat)
            params = [g.to(device=p.device, dtype=p.dtype)
                      for g, p in zip(grads, [p for _, p in torch.nn.Module.named_parameters(ctx.model)])]
        pos_t, lat_t = ctx.inputs
        din = (_as_input_grad(None if dpos is None else torch.from_numpy(dpos), pos_t),
               _as_input_grad(None if dlat is None else torch.from_numpy(dlat), lat_t))
        if ctx.model._device_training:
            return (None, None, None, *din, None)  # (the anchor)
        return (None, None, None, *din, *params)


class _TrainStepOnDevice(torch.autograd.Function):
    """``PotGNN.forward`` in training mode on CUDA tensors with ``DeviceAdam``: the batch, the result, the cotangents and
    the parameter gradients all stay in HBM (``rn_potgnn_train_forward_samples_device`` /
    ``rn_potgnn_train_backward_samples_device``); ``anchor`` only gives autograd a reason to call ``backward``."""

    @staticmethod
    def forward(ctx, model, lat_t, zs_t, pos_t, anchor):  # pylint: disable=arguments-differ,unused-argument
        ctx.model = model
        ctx.inputs = (pos_t.detach(), lat_t.detach())  # (shape, dtype and device of their gradients)
        return model._train_forward_on_device(lat_t, zs_t, pos_t)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # pylint: disable=arguments-differ
        want_lat, want_pos = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        dpos, dlat = ctx.model._train_backward_on_device(grad_out, want_pos, want_lat)
        pos_t, lat_t = ctx.inputs
        return (None, _as_input_grad(dlat, lat_t), None, _as_input_grad(dpos, pos_t), None)


class _DeviceSpan:  # pylint: disable=too-few-public-methods
    """``__cuda_array_interface__`` carrier for a float32 range of library-owned device memory."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f4", "data": (ptr, False),
                                         "version": 3, "strides": None}


def _alias_device_buffer(ptr: int, count: int, device_index: int) -> torch.Tensor:
    return torch.as_tensor(_DeviceSpan(ptr, count), device=torch.device("cuda", device_index))


class DeviceAdam:
    """``torch.optim.Adam`` (no amsgrad) applied where the weights live.  Constructing it switches
    the model to device-resident training; ``step()`` is one ``rn_potgnn_adam_step`` (Adam on the
    packed weights, refresh of everything derived from them), ``zero_grad()`` is a no-op (each
    backward overwrites the gradient buffer).  Drop-in for the optimiser argument of
    ``train_single_epoch`` (``pmodel/torch/_train.py:63-76``)."""

    def __init__(self, model: PotGNN, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        self.model = model
        self.param_groups = [dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                  weight_decay=float(weight_decay))]
        self.steps = 0
        model.enable_device_training(True)

    def step(self) -> None:
        group = self.param_groups[0]
        self.steps += 1
        self.model._adam_step(group["lr"], group["betas"][0], group["betas"][1], group["eps"],
                              group["weight_decay"], self.steps)

    def zero_grad(self, set_to_none: bool = True) -> None:  # pylint: disable=unused-argument
        return None
