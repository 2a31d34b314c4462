"""AMGX_MULTI_FUSE without a GPU: the flag's value, the fuse= keyword's validation (before any native call) and the
null-handle answers of the two new entry points."""
import ctypes as C

import numpy as np
import pytest

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError


def test_flag_value_and_symbols():
    assert _lib.AMGX_MULTI_FUSE == 64
    assert _lib.AMGX_MULTI_FUSE & (_lib.AMGX_DEVICE_PTR | _lib.AMGX_NO_GRAPH | _lib.AMGX_PCG_SINGLE_REDUCTION | _lib.AMGX_MULTI_INTERLEAVED) == 0
    assert "amgx_multi_plan" in _lib.AMGX_SYMBOLS and "amgx_multi_note" in _lib.AMGX_SYMBOLS


class _NoLibrary:
    """stands where the loaded library would: any access means the call got past the argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_matrix():
    from ngsamg_amd.device import DeviceAMGMatrix
    dev = object.__new__(DeviceAMGMatrix)
    dev._lib = _NoLibrary()
    dev._h = None
    dev.sizes = [4]
    dev.ext_sizes = [4]
    return dev


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0, [True]])
def test_fuse_must_be_a_boolean(bad):
    from ngsamg_amd.device import check_fuse
    from ngsamg_amd.krylov import NativeCGSolver
    assert check_fuse(False) == 0 and check_fuse(True) == 64 and check_fuse(np.bool_(True)) == 64
    with pytest.raises(NgsAMGError, match="fuse"):
        check_fuse(bad)
    dev = _bare_matrix()
    B, X = np.zeros((2, 4)), np.zeros((2, 4))
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.MultMulti(B, X, fuse=bad)
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.MatVecMulti(0, B, X, fuse=bad)
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.multi_plan(2, fuse=bad)
    sol = object.__new__(NativeCGSolver)
    sol.mat, sol.tol, sol.maxsteps, sol.use_pre = dev, 1e-8, 10, True
    with pytest.raises(NgsAMGError, match="fuse"):
        sol.SolveMulti(B, X, fuse=bad)


def test_null_handle_is_an_error_not_a_crash():
    lib = _lib.hip()
    fused, ng, wb = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    wd = (C.c_int32 * _lib.AMGX_MULTI_MAX)()
    for flags in (0, _lib.AMGX_MULTI_FUSE):
        assert lib.amgx_multi_plan(None, 4, flags, C.byref(fused), C.byref(ng), wd, C.byref(wb)) != 0
        assert (fused.value, ng.value, wb.value) == (-7, -7, -7)
        note = lib.amgx_multi_note(None, flags)
        assert note is not None and b"null handle" in note
