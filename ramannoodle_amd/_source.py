"""Where the input of an analysis entry is: a host array, or a CUDA tensor that the library reads in place.  For the
modules whose functions take either (``lineshape``, ``peakfit``, ``quasiharmonic``, ``bandmodes``); it imports torch
only once it has been handed a tensor, which is why it does not live in ``pmodel/_device.py``."""
from __future__ import annotations

import numpy as np


def is_tensor(value) -> bool:
    return type(value).__module__.split(".")[0] == "torch"


def source(value, refusal: str):
    """``(pointer, device_index, stream, keepalive)`` of ``value``.  A contiguous float64 CUDA tensor: its pointer, its
    GPU and torch's current stream there (the ``_device`` entry orders its reads after it); any other tensor raises
    ``ValueError(refusal)``.  Anything else becomes a contiguous float64 host array: ``device_index`` and ``stream`` are
    ``None`` (the host entry).  ``keepalive`` is the tensor or the array: it owns the memory and carries the shape."""
    if not is_tensor(value):
        host = np.ascontiguousarray(value, dtype=np.float64)
        return host.ctypes.data, None, None, host
    import torch
    if not (value.is_cuda and value.is_contiguous() and value.dtype == torch.float64):
        raise ValueError(refusal)
    return value.data_ptr(), value.device.index or 0, torch.cuda.current_stream(value.device).cuda_stream, value
