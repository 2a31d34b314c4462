"""AMGX_MULTI_FUSE_DOWN_DIA without a GPU: the flag's value, the three new words of the fuse= keyword beside every
old value, the near misses, the way of the words through the multi-vector calls (before any native call) and the header's text."""
import os

import numpy as np
import pytest

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_and_disjoint_bits():
    assert _lib.AMGX_MULTI_FUSE_DOWN_DIA == 1024
    bits = [_lib.AMGX_DEVICE_PTR, _lib.AMGX_NO_GRAPH, _lib.AMGX_PCG_SINGLE_REDUCTION, _lib.AMGX_MULTI_INTERLEAVED, _lib.AMGX_MULTI_FUSE,
            _lib.AMGX_MULTI_FUSE_GS, _lib.AMGX_MULTI_FUSE_GS_BLOCK, _lib.AMGX_MULTI_FUSE_DOWN, _lib.AMGX_MULTI_FUSE_DOWN_DIA]
    for i, a in enumerate(bits):
        assert a > 0 and a & (a - 1) == 0, a                # one bit each
        for b in bits[i + 1:]:
            assert a & b == 0, (a, b)


def test_check_fuse_new_words_and_every_old_value():
    from ngsamg_amd.device import check_fuse
    assert check_fuse("down_dia") == 64 | 512 | 1024
    assert check_fuse("gs+down_dia") == 192 | 512 | 1024
    assert check_fuse("gs_block+down_dia") == 448 | 512 | 1024
    for word in ("down", "gs+down", "gs_block+down"):        # the bits of the word without "_dia", plus 1024
        assert check_fuse(word + "_dia") == check_fuse(word) | _lib.AMGX_MULTI_FUSE_DOWN_DIA
    # what was accepted stays accepted, with the same bits
    assert check_fuse(False) == 0 and check_fuse(True) == 64
    assert check_fuse(np.bool_(False)) == 0 and check_fuse(np.bool_(True)) == 64
    assert check_fuse("gs") == 192 and check_fuse("gs_block") == 448
    assert check_fuse("down") == 576 and check_fuse("gs+down") == 704 and check_fuse("gs_block+down") == 960
    # what was refused stays refused, and the near misses of the new words are refused too
    for bad in ("GS", "hgs", "", "true", "gs ", b"gs", "yes", None, 1, 0, 64, 192, "gs_block ", "block",
                "Down", "down ", "gs_down", "gs+", 512, 576, "down+gs", "+down", b"down",
                "down_dia ", "Down_dia", "dia", "down+dia", 1024, 1536, b"down_dia", "gs_dia", "gs+dia", "down_dia+gs", "_dia", 1600):
        with pytest.raises(NgsAMGError, match="fuse"):
            check_fuse(bad)


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


WORDS = ("down_dia", "gs+down_dia", "gs_block+down_dia")


def test_the_new_words_pass_through_the_multi_vector_calls():
    from ngsamg_amd.multivector import MatVecMulti, MultMulti
    dev = _bare_matrix()
    ok = np.ones((2, 6))
    for fuse in WORDS:
        assert MultMulti(dev, fuse=fuse).fuse == fuse and MatVecMulti(0, dev, fuse=fuse).fuse == fuse
        with pytest.raises(AssertionError, match="amgx_apply_multi"):
            dev.MultMulti(ok, np.zeros((2, 6)), fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_matvec_multi"):
            dev.MatVecMulti(0, ok, np.zeros((2, 6)), fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_multi_plan"):
            dev.multi_plan(4, fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_multi_level_plan"):
            dev.multi_level_plan(0, fuse=fuse)
        with pytest.raises(AssertionError, match="amgx_down_multi"):
            dev.DownMulti(0, ok, fuse=fuse)
    for bad in ("down_dia ", "Down_dia", "dia", "down+dia", 1024, 1536, b"down_dia"):
        with pytest.raises(NgsAMGError, match="fuse"):
            MultMulti(dev, fuse=bad)
        with pytest.raises(NgsAMGError, match="fuse"):
            dev.multi_level_plan(0, fuse=bad)
        with pytest.raises(NgsAMGError, match="fuse"):
            dev.DownMulti(0, ok, fuse=bad)


def test_the_level_plan_forms_name_the_two_new_kernels():
    from ngsamg_amd.device import DeviceAMGMatrix
    assert DeviceAMGMatrix._LEVEL_PLAN_FORMS == ("literal", "sell", "sell-win", "dia", "dia-box")


def test_header_names_the_flag_in_the_enum_and_in_the_multi_vector_block():
    text = open(os.path.join(ROOT, "include", "amgx.h")).read()
    enum = text[text.index("AMGX_MULTI_FUSE_DOWN = 512"):text.index("typedef struct amgx_level_desc")]
    assert "AMGX_MULTI_FUSE_DOWN_DIA = 1024" in enum             # the enumerator follows AMGX_MULTI_FUSE_DOWN
    start = text.index("---- multi-vectors: k right-hand sides per matrix pass")
    end = text.index("---- multi-vector algebra")
    block = text[start:end]
    assert block.index("AMGX_MULTI_FUSE_DOWN = 512") < block.index("AMGX_MULTI_FUSE_DOWN_DIA = 1024")
    tail = block[block.index("AMGX_MULTI_FUSE_DOWN_DIA = 1024"):]
    for phrase in ('"dia"', '"dia-box"', "x = z + Q x_c", '"diagonal image" remains the note', '"local-window image"', "3 diagonal image on 512-row chunks",
                   "4 diagonal image on box chunks"):
        assert phrase in tail, phrase
