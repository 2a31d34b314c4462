"""AMGX_MULTI_FUSE_GS_BLOCK without a GPU: the flag's value, fuse="gs_block" in the keyword's validation, the
header's text and the shape checks of SmoothMulti / MultMulti (before any native call)."""
import os

import numpy as np
import pytest

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_and_disjoint_bits():
    assert _lib.AMGX_MULTI_FUSE_GS_BLOCK == 256
    bits = [_lib.AMGX_DEVICE_PTR, _lib.AMGX_NO_GRAPH, _lib.AMGX_PCG_SINGLE_REDUCTION, _lib.AMGX_MULTI_INTERLEAVED, _lib.AMGX_MULTI_FUSE,
            _lib.AMGX_MULTI_FUSE_GS, _lib.AMGX_MULTI_FUSE_GS_BLOCK]
    for i, a in enumerate(bits):
        assert a > 0 and a & (a - 1) == 0, a                # one bit each
        for b in bits[i + 1:]:
            assert a & b == 0, (a, b)


def test_check_fuse_values():
    from ngsamg_amd.device import check_fuse
    assert check_fuse("gs_block") == 448 == _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS | _lib.AMGX_MULTI_FUSE_GS_BLOCK
    # what the keyword answered before stays
    assert check_fuse(False) == 0 and check_fuse(True) == 64 and check_fuse(np.bool_(True)) == 64 and check_fuse("gs") == 192
    for bad in ("GS_BLOCK", "gs-block", "gsblock", "gs_block ", " gs_block", "block", "gs_blocks", b"gs_block", 448, 256, None,
                "GS", "hgs", "", "true", "gs ", b"gs"):
        with pytest.raises(NgsAMGError, match="fuse"):
            check_fuse(bad)


def test_null_handle_is_an_error_under_the_flag():
    lib = _lib.hip()
    x, b = np.zeros(8), np.ones(8)
    for flags in (_lib.AMGX_MULTI_FUSE_GS_BLOCK, 448):
        assert lib.amgx_smooth_multi(None, 0, 0, 2, x.ctypes.data, 4, b.ctypes.data, 4, 0, flags) != 0
        assert not x.any()
        note = lib.amgx_multi_note(None, flags)
        assert note is not None and b"null handle" in note


def test_header_names_the_flag_in_the_multi_vector_block():
    text = open(os.path.join(ROOT, "include", "amgx.h")).read()
    assert "AMGX_MULTI_FUSE_GS_BLOCK = 256" in text
    assert "AMGX_MULTI_FUSE_GS = 128" in text
    start = text.index("---- multi-vectors: k right-hand sides per matrix pass")
    end = text.index("---- multi-vector algebra")
    block = text[start:end]
    assert block.index("AMGX_MULTI_FUSE_GS_BLOCK") > block.index("AMGX_MULTI_FUSE_GS ")       # documented next to (after) the scalar flag
    for words in ("block size 2, 3 or 6", "hybrid-block", "block-coloured", "row-list", "sweep block too large for the multi-vector sweep",
                  "bit for bit", "AMGX_SM_BGS", "ProxySmoother", "rank-partitioned", "Gauss-Seidel on a block level"):
        assert words in block, words
    assert "int amgx_smooth_multi(amgx_handle h, int level, int dir, int k," in block


class _NoLibrary:
    """stands where the loaded library would: any access means the call got past the argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_matrix():
    from ngsamg_amd.device import DeviceAMGMatrix
    dev = object.__new__(DeviceAMGMatrix)
    dev._lib = _NoLibrary()
    dev._h = None
    dev.n_levels = 2
    dev.sizes = [6, 3]
    dev.ext_sizes = [6, 5]
    return dev


def test_shapes_are_checked_before_the_library_is_called():
    dev = _bare_matrix()
    ok = np.zeros((2, 6))
    cases = [(np.zeros((2, 5)), ok, False),                 # wrong number of rows
             (ok, np.zeros((3, 6)), False),                 # different numbers of columns
             (np.zeros((6, 2)), np.zeros((6, 2)), False),   # interleaved data without the keyword
             (ok, ok, True),                                # ... and the other way round
             (np.zeros((9, 6)), np.zeros((9, 6)), False),   # more than AMGX_MULTI_MAX columns
             (np.zeros(6), np.zeros(6), False),             # not 2-D
             (np.zeros((2, 6), dtype=np.float32), ok, False)]
    for X, B, il in cases:
        with pytest.raises(NgsAMGError):
            dev.SmoothMulti(0, X, B, interleaved=il, fuse="gs_block")
        with pytest.raises(NgsAMGError):
            dev.MultMulti(B, X, interleaved=il, fuse="gs_block")
    with pytest.raises(NgsAMGError, match="level"):
        dev.SmoothMulti(2, ok, ok, fuse="gs_block")
    with pytest.raises(NgsAMGError, match="ghost"):
        dev.SmoothMulti(1, np.zeros((2, 3)), np.zeros((2, 3)), fuse="gs_block")
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.SmoothMulti(0, ok, ok, fuse="gs_blok")
    # a valid call reaches the library (and only then)
    with pytest.raises(AssertionError, match="amgx_smooth_multi"):
        dev.SmoothMulti(0, ok, np.ones((2, 6)), fuse="gs_block")
    with pytest.raises(AssertionError, match="amgx_apply_multi"):
        dev.MultMulti(np.ones((2, 6)), ok, fuse="gs_block")
    with pytest.raises(AssertionError, match="amgx_multi_plan"):
        dev.multi_plan(4, fuse="gs_block")
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.multi_plan(4, fuse="gs_blok")


def test_block_operators_and_solvers_keep_the_keyword():
    from ngsamg_amd.krylov import NativeCGSolver
    from ngsamg_amd.multivector import MatVecMulti, MultMulti
    dev = _bare_matrix()
    assert MultMulti(dev, fuse="gs_block").fuse == "gs_block" and MatVecMulti(0, dev, fuse="gs_block").fuse == "gs_block"
    with pytest.raises(NgsAMGError, match="fuse"):
        MultMulti(dev, fuse="block")
    cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=5)
    with pytest.raises(NgsAMGError, match="fuse"):
        cg.SolveMulti(np.ones((2, 6)), np.zeros((2, 6)), fuse="gs_blok")
    with pytest.raises(AssertionError, match="amgx_pcg_multi"):       # a valid keyword gets past the checks
        cg.SolveMulti(np.ones((2, 6)), np.zeros((2, 6)), fuse="gs_block")
