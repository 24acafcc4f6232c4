"""irt_update_values*: what needs no GPU -- the exported symbols, the NULL-context answers, and
the binding's argument check."""
import ctypes as C

import numpy as np
import pytest

import irt

NAMES = ("irt_update_values", "irt_update_values_device", "irt_update_values_end")


def test_library_exports_the_update_calls():
    lib = C.CDLL(irt.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_null_context_is_invalid_before_any_device_call():
    L = irt.lib()
    vals = np.zeros((2, 32), np.float32)
    assert L.irt_update_values(None, 0, 2, vals.ctypes.data) == irt.E_INVALID
    assert b"irt_update_values" in L.irt_last_error()
    assert L.irt_update_values(None, 0, 0, None) == irt.E_INVALID
    assert L.irt_update_values_device(None, 0, 2, vals.ctypes.data, None) == irt.E_INVALID
    assert b"irt_update_values_device" in L.irt_last_error()
    assert L.irt_update_values_end(None) == irt.E_INVALID
    assert b"irt_update_values_end" in L.irt_last_error()


def test_binding_checks_the_values_array():
    ok = np.zeros((3, 32), np.float32)
    assert irt.check_update_values(ok) is ok  # passed on as it is: no copy, no conversion
    assert irt.check_update_values(np.zeros((0, 32), np.float32)).shape == (0, 32)
    with pytest.raises(TypeError):
        irt.check_update_values(np.zeros((3, 32), np.float64))
    with pytest.raises(TypeError):
        irt.check_update_values([[0.0] * 32])
    for bad in (np.zeros(32, np.float32), np.zeros((3, 31), np.float32), np.zeros((3, 32, 1), np.float32)):
        with pytest.raises(ValueError):
            irt.check_update_values(bad)
    with pytest.raises(ValueError):
        irt.check_update_values(np.zeros((32, 3), np.float32).T)  # right shape, not C-contiguous
    with pytest.raises(ValueError):
        irt.check_update_values(np.zeros((3, 64), np.float32)[:, ::2])
