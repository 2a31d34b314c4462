"""Multi-vector calls (k right-hand sides per matrix pass), the part that needs no GPU: argument validation of the Python layer,
the native calls on a NULL handle, and the exported symbols with their ctypes signatures."""
import ctypes as C

import numpy as np
import pytest

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError
from ngsamg_amd.device import check_multi

N = 11


def test_check_multi_accepts_both_layouts():
    B, X = np.zeros((3, N)), np.zeros((3, N))
    k, addrs, lds, dev = check_multi((B, X), (N, N))
    assert (k, lds, dev) == (3, [N, N], False) and addrs == [B.ctypes.data, X.ctypes.data]
    Bi, Xi = np.zeros((N, 8)), np.zeros((N, 8))
    k, addrs, lds, dev = check_multi((Bi, Xi), (N, N), interleaved=True)
    assert k == 8 and not dev
    # different row counts per argument (MatVecMulti on a level with ghost columns)
    k, _, lds, _ = check_multi((np.zeros((2, N + 3)), np.zeros((2, N))), (N + 3, N))
    assert k == 2 and lds == [N + 3, N]


@pytest.mark.parametrize("B,X,il,msg", [
    (np.zeros((0, N)), np.zeros((0, N)), False, "right-hand sides"),                       # k = 0
    (np.zeros((9, N)), np.zeros((9, N)), False, "right-hand sides"),                       # k = 9
    (np.zeros((N, 9)), np.zeros((N, 9)), True, "right-hand sides"),                        # k = 9, interleaved
    (np.zeros((2, N + 1)), np.zeros((2, N)), False, "shape"),                              # wrong length
    (np.zeros((N, 2)), np.zeros((N, 2)), False, "right-hand sides|shape"),                 # interleaved data without the flag
    (np.zeros((2, N)), np.zeros((3, N)), False, "the other argument"),                     # k differs
    (np.zeros(N), np.zeros(N), False, "2-D"),                                              # 1-D
    (np.zeros((2, N), dtype=np.float32), np.zeros((2, N)), False, "float64"),              # wrong dtype
    (np.zeros((2, 2 * N))[:, ::2], np.zeros((2, N)), False, "contiguous"),                 # strided
    (np.zeros((N, 2)).T, np.zeros((2, N)), False, "contiguous"),                           # transposed view
    ([[0.0] * N] * 2, np.zeros((2, N)), False, "numpy array or CUDA tensor"),              # not an array
])
def test_check_multi_rejects(B, X, il, msg):
    with pytest.raises(NgsAMGError, match=msg):
        check_multi((B, X), (N, N), interleaved=il)


def test_check_multi_rejects_mixed_host_and_device():
    class FakeCuda:                      # what _is_torch looks for; never dereferenced: the kind check comes first
        is_cuda = True

        def data_ptr(self):
            return 0
    with pytest.raises(NgsAMGError, match="mixing host arrays and device tensors"):
        check_multi((FakeCuda(), np.zeros((2, N))), (N, N))
    import torch
    with pytest.raises(NgsAMGError, match="must live on the GPU"):
        check_multi((torch.zeros(2, N, dtype=torch.float64), torch.zeros(2, N, dtype=torch.float64)), (N, N))


def test_native_calls_with_null_handle_fail_with_a_message():
    lib = _lib.hip()
    b, x = np.ones((2, N)), np.zeros((2, N))
    errs, its = np.zeros(2 * 4), np.zeros(2, dtype=np.int32)
    fused, ng, wb = C.c_int32(), C.c_int32(), C.c_int64()
    wd = (C.c_int32 * _lib.AMGX_MULTI_MAX)()
    calls = {
        "amgx_apply_multi": lambda k: lib.amgx_apply_multi(None, k, b.ctypes.data, N, x.ctypes.data, N, 0, 0),
        "amgx_matvec_multi": lambda k: lib.amgx_matvec_multi(None, 0, k, b.ctypes.data, N, x.ctypes.data, N, 0),
        "amgx_pcg_multi": lambda k: lib.amgx_pcg_multi(None, k, b.ctypes.data, N, x.ctypes.data, N, 1e-8, 3, 1, 0,
                                                       errs.ctypes.data_as(_lib.c_f64p), its.ctypes.data_as(_lib.c_i32p)),
        "amgx_multi_info": lambda k: lib.amgx_multi_info(None, k, C.byref(fused), C.byref(ng), wd, C.byref(wb)),
    }
    for name, call in calls.items():
        for k in (1, 2):                 # k = 1 is the shortcut to the single-vector path: it must not dereference the handle either
            assert call(k) != 0, (name, k)
            msg = lib.amgx_last_error(None).decode()
            assert "null handle" in msg, (name, k, msg)
    assert np.all(x == 0.0)


def test_symbols_exported_with_signatures():
    lib = _lib.hip()
    arity = {"amgx_apply_multi": 8, "amgx_matvec_multi": 8, "amgx_pcg_multi": 12, "amgx_multi_info": 6}
    for name, n in arity.items():
        assert name in _lib.AMGX_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    assert _lib.AMGX_MULTI_MAX == 8 and _lib.AMGX_MULTI_INTERLEAVED == 32
    # the flag bit is free of the other public flags
    assert _lib.AMGX_MULTI_INTERLEAVED & (_lib.AMGX_DEVICE_PTR | _lib.AMGX_NO_GRAPH | _lib.AMGX_PCG_SINGLE_REDUCTION) == 0
    import re, os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amgx.h")).read()
    assert re.search(r"#define\s+AMGX_MULTI_MAX\s+8\b", hdr) and re.search(r"AMGX_MULTI_INTERLEAVED\s*=\s*32\b", hdr)


def test_python_surface_exists():
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.krylov import NativeCGSolver
    from ngsamg_amd import NgsAMG
    for cls, names in ((DeviceAMGMatrix, ("MultMulti", "MatVecMulti", "multi_info")), (NativeCGSolver, ("SolveMulti",)),
                       (NgsAMG.AMGMatrix, ("MultMulti",)), (NgsAMG._AMGPreconditioner, ("MultMulti",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
