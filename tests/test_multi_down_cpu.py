"""AMGX_MULTI_FUSE_DOWN without a GPU: the flag's value, the three new words of the fuse= keyword beside every old
value, the declarations of amgx_down_multi / amgx_multi_level_plan / amgx_multi_level_note, the header's text and the argument
checks of DownMulti / multi_level_plan (before any native call)."""
import ctypes as C
import os

import numpy as np
import pytest

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_and_disjoint_bits():
    assert _lib.AMGX_MULTI_FUSE_DOWN == 512
    bits = [_lib.AMGX_DEVICE_PTR, _lib.AMGX_NO_GRAPH, _lib.AMGX_PCG_SINGLE_REDUCTION, _lib.AMGX_MULTI_INTERLEAVED, _lib.AMGX_MULTI_FUSE,
            _lib.AMGX_MULTI_FUSE_GS, _lib.AMGX_MULTI_FUSE_GS_BLOCK, _lib.AMGX_MULTI_FUSE_DOWN]
    for i, a in enumerate(bits):
        assert a > 0 and a & (a - 1) == 0, a                # one bit each
        for b in bits[i + 1:]:
            assert a & b == 0, (a, b)


def test_check_fuse_new_words_and_every_old_value():
    from ngsamg_amd.device import check_fuse
    assert check_fuse("down") == 64 | 512
    assert check_fuse("gs+down") == 192 | 512
    assert check_fuse("gs_block+down") == 448 | 512
    # what was accepted stays accepted, with the same bits
    assert check_fuse(False) == 0 and check_fuse(True) == 64
    assert check_fuse(np.bool_(False)) == 0 and check_fuse(np.bool_(True)) == 64
    assert check_fuse("gs") == 192 and check_fuse("gs_block") == 448
    # what was refused stays refused, and the near misses of the new words are refused too
    for bad in ("GS", "hgs", "", "true", "gs ", b"gs", "yes", None, 1, 0, 64, 192, "gs_block ", "block",
                "Down", "down ", "gs_down", "gs+", 512, 576, "down+gs", "+down", b"down"):
        with pytest.raises(NgsAMGError, match="fuse"):
            check_fuse(bad)


def test_the_three_symbols_are_declared():
    for name in ("amgx_down_multi", "amgx_multi_level_plan", "amgx_multi_level_note"):
        assert name in _lib.AMGX_SYMBOLS
    lib = _lib.hip()
    vp, i64 = C.c_void_p, C.c_int64
    assert lib.amgx_down_multi.argtypes == [vp, C.c_int, C.c_int, vp, i64, vp, i64, vp, i64, C.c_int, C.c_int]
    assert lib.amgx_multi_level_plan.argtypes == [vp, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]
    assert lib.amgx_multi_level_note.argtypes == [vp, C.c_int, C.c_int] and lib.amgx_multi_level_note.restype == C.c_char_p
    # a null handle is an error, not a crash, and nothing is written
    b, x, bc = np.ones(8), np.zeros(8), np.zeros(4)
    assert lib.amgx_down_multi(None, 0, 2, b.ctypes.data, 4, x.ctypes.data, 4, bc.ctypes.data, 2, 0, _lib.AMGX_MULTI_FUSE_DOWN) != 0
    assert not x.any() and not bc.any()
    out = (C.c_int32 * 5)(7, 7, 7, 7, 7)
    assert lib.amgx_multi_level_plan(None, 0, _lib.AMGX_MULTI_FUSE_DOWN, out, 5) != 0
    assert list(out) == [7] * 5
    note = lib.amgx_multi_level_note(None, 0, _lib.AMGX_MULTI_FUSE_DOWN)
    assert note is not None and b"null handle" in note


def test_header_names_the_flag_and_the_calls_in_the_multi_vector_block():
    text = open(os.path.join(ROOT, "include", "amgx.h")).read()
    assert "AMGX_MULTI_FUSE_DOWN = 512" in text
    enum = text[text.index("AMGX_MULTI_FUSE_GS_BLOCK = 256"):text.index("typedef struct amgx_level_desc")]
    assert "AMGX_MULTI_FUSE_DOWN = 512" in enum                # the enumerator follows AMGX_MULTI_FUSE_GS_BLOCK
    start = text.index("---- multi-vectors: k right-hand sides per matrix pass")
    end = text.index("---- multi-vector algebra")
    block = text[start:end]
    assert block.index("AMGX_MULTI_FUSE_GS_BLOCK") < block.index("AMGX_MULTI_FUSE_DOWN = 512")
    assert "int amgx_down_multi(amgx_handle h, int level, int k, const double* B, int64_t ldb, double* X, int64_t ldx, double* BC, int64_t ldbc," in block
    assert "int amgx_multi_level_plan(amgx_handle h, int level, int flags, int32_t* out, int n_out);" in block
    assert "const char* amgx_multi_level_note(amgx_handle h, int level, int flags);" in block
    for reason in ("local-window image", "diagonal image", "workgroup size", "no chunk-local restriction", "block level", "multicolour sweep"):
        assert '"' + reason + '"' in block, reason


class _NoLibrary:
    """stands where the loaded library would: any access means the call got past the argument checks"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_matrix():
    from ngsamg_amd.device import DeviceAMGMatrix
    dev = object.__new__(DeviceAMGMatrix)
    dev._lib = _NoLibrary()
    dev._h = None
    dev.n_levels = 3
    dev.sizes = [6, 3, 2]
    dev.ext_sizes = [6, 5, 2]
    return dev


def test_down_multi_checks_its_arguments_before_the_library_is_called():
    dev = _bare_matrix()
    ok = np.ones((2, 6))
    cases = [(np.zeros((2, 5)), np.zeros((2, 5)), False),   # wrong number of rows
             (ok, np.zeros((3, 6)), False),                 # different numbers of columns
             (np.zeros((6, 2)), np.zeros((6, 2)), False),   # interleaved data without the keyword
             (ok, np.zeros((2, 6)), True),                  # ... and the other way round
             (np.zeros((9, 6)), np.zeros((9, 6)), False),   # more than AMGX_MULTI_MAX columns
             (np.zeros(6), np.zeros(6), False),             # not 2-D
             (np.zeros((2, 6), dtype=np.float32), np.zeros((2, 6)), False),
             (ok, np.zeros((2, 6), dtype=np.float32), False)]
    for B, X, il in cases:
        for given in (False, True):
            with pytest.raises(NgsAMGError):
                dev.DownMulti(0, B, X, x_given=given, interleaved=il, fuse="down")
    with pytest.raises(NgsAMGError):
        dev.DownMulti(0, np.zeros((2, 5)), fuse="down")       # X=None: B alone is checked the same way
    with pytest.raises(NgsAMGError, match="level"):
        dev.DownMulti(3, ok, fuse="down")
    with pytest.raises(NgsAMGError, match="level"):
        dev.DownMulti(-1, ok, fuse="down")
    with pytest.raises(NgsAMGError, match="coarsest"):
        dev.DownMulti(2, np.ones((2, 2)), fuse="down")
    with pytest.raises(NgsAMGError, match="ghost"):
        dev.DownMulti(1, np.ones((2, 3)), fuse="gs+down")
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.DownMulti(0, ok, fuse="Down")
    with pytest.raises(NgsAMGError, match="fuse"):
        dev.DownMulti(0, ok, fuse=512)
    with pytest.raises(NgsAMGError, match="x_given"):
        dev.DownMulti(0, ok, np.zeros((2, 6)), x_given=1)
    with pytest.raises(NgsAMGError, match="x_given"):
        dev.DownMulti(0, ok, x_given=True)                    # an iterate that is given has to be passed
    with pytest.raises(NgsAMGError, match="level"):
        dev.DownMulti(0.0, ok)
    # a valid call reaches the library (and only then), with and without the bit
    for fuse in (False, True, "down", "gs+down", "gs_block+down"):
        with pytest.raises(AssertionError, match="amgx_down_multi"):
            dev.DownMulti(0, ok, fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_down_multi"):
            dev.DownMulti(0, ok, np.zeros((2, 6)), x_given=True, fuse=fuse)
    with pytest.raises(AssertionError, match="amgx_down_multi"):
        dev.DownMulti(0, np.ones((6, 2)), interleaved=True, fuse="down")


def test_multi_level_plan_checks_its_arguments_before_the_library_is_called():
    dev = _bare_matrix()
    for level in (-1, 3, 99):
        with pytest.raises(NgsAMGError, match="level"):
            dev.multi_level_plan(level, fuse="down")
    for level in (0.5, "0", None, True):
        with pytest.raises(NgsAMGError, match="level"):
            dev.multi_level_plan(level, fuse="down")
    for bad in ("Down", "down ", "gs_down", "gs+", 512, 576):
        with pytest.raises(NgsAMGError, match="fuse"):
            dev.multi_level_plan(0, fuse=bad)
    for fuse in (False, True, "gs", "down", "gs+down", "gs_block+down"):
        with pytest.raises(AssertionError, match="amgx_multi_level_plan"):
            dev.multi_level_plan(0, fuse=fuse)


def test_the_new_words_pass_through_the_other_multi_vector_calls():
    from ngsamg_amd.multivector import MatVecMulti, MultMulti
    dev = _bare_matrix()
    ok = np.ones((2, 6))
    for fuse in ("down", "gs+down", "gs_block+down"):
        assert MultMulti(dev, fuse=fuse).fuse == fuse and MatVecMulti(0, dev, fuse=fuse).fuse == fuse
        with pytest.raises(AssertionError, match="amgx_apply_multi"):
            dev.MultMulti(ok, np.zeros((2, 6)), fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_multi_plan"):
            dev.multi_plan(4, fuse=fuse)
    with pytest.raises(NgsAMGError, match="fuse"):
        MultMulti(dev, fuse="gs_down")
