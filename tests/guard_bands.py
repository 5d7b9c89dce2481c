"""Guard bands for the device-pointer entries (tests/test_guard_bands.py, tests/test_guard_bands_gpu.py): an array handed
to an entry as a contiguous view in the middle of a larger buffer whose two ends hold a known bit pattern.  A load past
an end of an input then returns NaN, so that it shows in the result; a store past an end of an output changes a band,
which ``assert_bands_intact`` reports by its offset from the view; a result element that the entry never wrote still
holds the pre-fill (``assert_overwritten``).  Either way the overrun lands in memory the test owns.

``lead`` is the number of elements in front of the view: ``ALIGNED`` (4096) keeps the 512-byte alignment of a torch
allocation, ``ODD`` (4097) leaves the view aligned to its element size only.  A plain module: no conftest, no pytest
settings."""
import contextlib

import numpy as np
import torch

ALIGNED = 4096
ODD = 4097
LEADS = (ALIGNED, ODD)

NAN = "nan"  # the fill of input bands: the canonical quiet NaN of the type (zero for integer types, a valid index)
# bands of outputs and the pre-fill of their interior: two NaNs with distinct payloads, so that neither is ever a
# computed value and each is told from the other and from a canonical NaN by its bits
_BAND_BITS = {8: 0x7FF85EA7BAADF00D, 4: 0x7FC5EA7B}
_PREFILL_BITS = {8: 0x7FF80DD5C0DED00D, 4: 0x7FC0DD5C}
SENTINEL = "sentinel"

_INT_OF_SIZE = {8: np.int64, 4: np.int32}
_TORCH_INT_OF_SIZE = {8: torch.int64, 4: torch.int32}


class HostBuffer(np.ndarray):
    """A numpy buffer that remembers its band fill (``guard_fill``, as signed integer bits)."""
    guard_fill = None


def _signed(bits: int, size: int) -> int:
    return bits - (1 << (8 * size)) if bits >= 1 << (8 * size - 1) else bits


def _numpy_dtype(dtype) -> np.dtype:
    if isinstance(dtype, torch.dtype):
        return np.dtype({torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32,
                         torch.int64: np.int64}[dtype])
    return np.dtype(dtype)


def fill_bits(dtype, fill) -> int:
    """The signed integer whose bits are ``fill`` in ``dtype``: ``NAN``, ``SENTINEL`` or an integer bit pattern."""
    dtype = _numpy_dtype(dtype)
    if fill == NAN:
        if dtype.kind != "f":
            return 0
        return int(np.array(np.nan, dtype=dtype).view(_INT_OF_SIZE[dtype.itemsize]))
    if fill == SENTINEL:
        fill = _BAND_BITS[dtype.itemsize]
    return _signed(int(fill), dtype.itemsize)


def prefill_bits(dtype) -> int:
    dtype = _numpy_dtype(dtype)
    return _signed(_PREFILL_BITS[dtype.itemsize], dtype.itemsize)


def banded(values_or_shape, dtype, lead, fill, device=None, row=0):
    """``(buffer, view)``: ``view`` is ``buffer[band : band + numel]`` in the wanted shape with ``band = max(lead, row)``
    rounded so that ``band - lead`` is a multiple of 64 elements (the alignment class of ``lead`` is kept), and as many
    elements behind it.  ``values_or_shape``: an array or tensor whose values the view takes (an input), or a shape,
    whose interior is then pre-filled with the second sentinel (an output).  ``device=None``: a numpy ``HostBuffer``;
    otherwise a torch tensor there.  ``row``: the longest tile row, in elements, that the entry's kernel could
    over-read or over-write."""
    np_dtype = _numpy_dtype(dtype)
    is_shape = isinstance(values_or_shape, (tuple, list, torch.Size)) and all(
        isinstance(n, (int, np.integer)) for n in values_or_shape)
    if is_shape:
        shape, values = tuple(int(n) for n in values_or_shape), None
    else:
        values = values_or_shape.detach().cpu().numpy() if isinstance(values_or_shape, torch.Tensor) \
            else np.asarray(values_or_shape)
        values = np.ascontiguousarray(values, dtype=np_dtype)
        shape = values.shape
    numel = int(np.prod(shape, dtype=np.int64))
    band = int(lead) + (-(-max(int(row) - int(lead), 0) // 64)) * 64
    bits = fill_bits(np_dtype, fill)
    as_int = _INT_OF_SIZE[np_dtype.itemsize]
    host = np.full(2 * band + numel, bits, dtype=as_int)
    host[band:band + numel] = prefill_bits(np_dtype) if values is None else values.reshape(-1).view(as_int)
    if device is None:
        buffer = host.view(np_dtype).view(HostBuffer)
        buffer.guard_fill = bits
        view = np.asarray(buffer)[band:band + numel].reshape(shape)
        return buffer, view
    buffer = torch.from_numpy(host).to(device).view(
        {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
         np.dtype(np.int64): torch.int64}[np_dtype])
    buffer.guard_fill = bits
    view = buffer[band:band + numel].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buffer.data_ptr() + band * np_dtype.itemsize
    return buffer, view


def _bits_and_lead(buffer, view):
    """``(the buffer as host integers, the offset of the view, its element count)``."""
    if isinstance(buffer, torch.Tensor):
        size = buffer.element_size()
        lead = (view.data_ptr() - buffer.data_ptr()) // size
        return buffer.view(_TORCH_INT_OF_SIZE[size]).cpu().numpy(), lead, view.numel()
    size = buffer.dtype.itemsize
    lead = (view.ctypes.data - buffer.ctypes.data) // size
    return np.asarray(buffer).view(_INT_OF_SIZE[size]), lead, view.size


def assert_bands_intact(buffer, view, what="array"):
    """Both bands of ``buffer`` still hold their fill, compared as integers (so NaN bands compare, payload included);
    otherwise an ``AssertionError`` naming the first changed element by its offset from the view."""
    bits, lead, numel = _bits_and_lead(buffer, view)
    fill = buffer.guard_fill
    behind = np.flatnonzero(bits[lead + numel:] != fill)
    front = np.flatnonzero(bits[:lead] != fill)
    if behind.size:
        at = int(behind[0])
        raise AssertionError(f"{what}: written +{at + 1} elements past the end ({behind.size} band elements changed; "
                             f"bits {int(bits[lead + numel + at]) & (2 ** (8 * bits.itemsize) - 1):#x})")
    if front.size:
        at = int(front[-1])
        raise AssertionError(f"{what}: written -{lead - at} elements before the start ({front.size} band elements "
                             f"changed; bits {int(bits[at]) & (2 ** (8 * bits.itemsize) - 1):#x})")


def interior_bits(buffer, view):
    """The view's elements as host integers, flat."""
    bits, lead, numel = _bits_and_lead(buffer, view)
    return bits[lead:lead + numel]


def assert_overwritten(buffer, view, what="output", untouched=None):
    """Every element of the view was written: none holds the pre-fill.  ``untouched``: a boolean mask of the view's
    shape of elements the entry promises to leave alone, which must all still hold the pre-fill."""
    bits = interior_bits(buffer, view)
    stale = bits == prefill_bits(view.dtype)
    if untouched is None:
        missed = np.flatnonzero(stale)
        assert missed.size == 0, f"{what}: {missed.size} elements never written, the first at flat index {int(missed[0])}"
        return
    untouched = np.asarray(untouched, dtype=bool).reshape(-1)
    missed = np.flatnonzero(stale & ~untouched)
    assert missed.size == 0, f"{what}: {missed.size} elements never written, the first at flat index {int(missed[0])}"
    touched = np.flatnonzero(~stale & untouched)
    assert touched.size == 0, (f"{what}: {touched.size} elements written that are documented as left alone, the first "
                               f"at flat index {int(touched[0])}")


class _BandedNumpy:
    """``numpy`` for a module of the package while a call runs: ``empty`` (and, when asked, ``zeros``) return banded
    views, so that the host results the module hands to a C entry by pointer lie between guard bands."""

    def __init__(self, lead, zeros):
        self._lead, self._zeros, self.results = lead, zeros, []

    def __getattr__(self, name):
        return getattr(np, name)

    def _banded(self, shape, dtype):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(n) for n in shape)
        buffer, view = banded(shape, dtype, self._lead, SENTINEL, row=shape[-1] if shape else 0)
        self.results.append((buffer, view))
        return view

    def empty(self, shape, dtype=np.float64):  # pylint: disable=missing-function-docstring
        return self._banded(shape, dtype)

    def zeros(self, shape, dtype=np.float64):  # pylint: disable=missing-function-docstring
        return self._banded(shape, dtype) if self._zeros else np.zeros(shape, dtype=dtype)


@contextlib.contextmanager
def banded_host_results(module, lead, zeros=False):
    """While the block runs, every ``np.empty`` (with ``zeros``: and ``np.zeros``) of ``module`` is a banded host buffer
    whose interior holds the pre-fill: the arrays a front end allocates for a C entry to fill.  Yields the list of
    ``(buffer, view)`` made so far."""
    proxy = _BandedNumpy(lead, zeros)
    real = module.np
    module.np = proxy
    try:
        yield proxy.results
    finally:
        module.np = real


def assert_same_bits(got, want, what="result"):
    """``got`` equals ``want`` bit for bit (arrays or tensors of one type and shape)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    as_int = _INT_OF_SIZE[got.dtype.itemsize]
    a, b = np.ascontiguousarray(got).reshape(-1).view(as_int), np.ascontiguousarray(want).reshape(-1).view(as_int)
    differ = np.flatnonzero(a != b)
    assert differ.size == 0, (f"{what}: {differ.size} of {a.size} elements differ from the plain call, the first at flat "
                              f"index {int(differ[0])}: {got.reshape(-1)[differ[0]]!r} != {want.reshape(-1)[differ[0]]!r}")
