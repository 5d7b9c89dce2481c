"""Argument checks of the input-gradient entries of the C ABI (``rn_potgnn_forward_vjp_device``,
``rn_potgnn_train_backward_inputs(_device)``): rejected before any device work, so these run without a GPU."""
import ctypes as C

from ramannoodle_amd import _lib


def test_input_gradient_entries_reject_a_null_handle():
    lib = _lib.load()
    buf = (C.c_double * 64)()
    f32 = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(f32, C.c_void_p)
    assert lib.rn_potgnn_forward_vjp_device(None, None, None, p, 1, p, 0, p, p, None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_forward_vjp_device(None, None, None, p, 0, p, 1, None, p, None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_train_backward_inputs(None, q, q, p, p) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_train_backward_inputs(None, q, None, p, None) == _lib.RN_ERR_INVALID_ARGUMENT
    assert lib.rn_potgnn_train_backward_inputs_device(None, q, p, p, None) == _lib.RN_ERR_INVALID_ARGUMENT


def test_input_gradient_entries_are_declared_with_their_signatures():
    for name, nargs in (("rn_potgnn_forward_vjp_device", 10), ("rn_potgnn_train_backward_inputs", 5),
                        ("rn_potgnn_train_backward_inputs_device", 5)):
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs, name
