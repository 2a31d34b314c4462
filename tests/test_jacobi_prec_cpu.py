"""Single-precision images for scalar Jacobi levels (jacobi_prec) without a GPU: the field, the enum and the query
in the header and in ctypes, the vocabulary of jacobi_prec in Python, the flag path through Preconditioner, and the numerics of the
definition on the CPU (tests/jacobi_prec_ref.py: the folded cycle with A' and Q rounded as stored) against the same cycle in fp64.

Measured here, on the problems tests/test_gpu_jacobi_prec.py runs (form of level 0: "apre" -- every entry of A' through float32, the
diagonal omega included, whose rounding has one sign on all rows --, "apre_wd" -- the diagonal slot carries omega dinv_i, on every
level --, "dia"; below level 0 "apre" unless stated; printed by the test):

    problem          change apre / apre_wd / dia        pcg 64 / 32   symmetry defect 64 / 32 (apre, apre_wd, dia)
    (6, 5, 70)       7.81e-08 / 2.77e-08 / 5.02e-08     34 / 34       8.9e-18 / 6.7e-10, 5.6e-10, 2.8e-10
    (9, 9, 9)        3.77e-08 / 2.26e-08 / 2.80e-08     13 / 13       4.0e-18 / 5.6e-10, 4.4e-10, 1.5e-10
    (7, 130)         6.15e-08 / 2.71e-08 / 4.56e-08     39 / 39       1.9e-17 / 9.3e-10, 1.1e-09, 5.7e-10
    (41, 37, 29)     8.46e-08 / 2.26e-08 / 6.99e-08     17 / 17       2.8e-18 / 6.9e-11, 9.1e-11, 1.1e-10

Rounding A' and Q independently leaves the cycle symmetric to float rounding only (defect up to 1.1e-9 against 1e-17); PCG to 1e-8 takes
the double cycle's iterations on all four, so all four are kept for the GPU test."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.jacobi_prec_ref import FoldedJacobiRef, symmetry_defect
from tests.mat_prec_ref import pcg
from tests.problems import elasticity_case, poisson_case, rhs, to_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the problems of tests/test_gpu_dia_box.py that the GPU test runs: (shape, Dirichlet, max_coarse_size)
PROBLEMS = [((6, 5, 70), "right|top", 10), ((9, 9, 9), "right|top", 10), ((7, 130), "left|top", 5), ((41, 37, 29), "right|top", 10)]
# the largest relative change of one application against the double cycle that the emulation may show here: A' and Q carry
# float-rounded entries (2^-24 = 6e-8 each, independent), a cycle adds ~10 of them per row over a handful of levels
CHANGE_MAX = 1e-7


def _header():
    with open(os.path.join(ROOT, "include", "amgx.h")) as f:
        return f.read()


# ---- 1. the interface ---------------------------------------------------------------------------------------------------------
def test_field_is_last_in_header_and_ctypes(tmp_path):
    from ngsamg_amd import _lib
    h = _header()
    body = h[h.index("typedef struct amgx_level_desc"):h.index("} amgx_level_desc;")]
    fields = re.findall(r"^\s*(?:const\s+)?[A-Za-z_0-9]+\*?\s+\*?([A-Za-z_0-9]+);", body, flags=re.M)
    assert fields[-2:] == ["mat_prec", "jacobi_prec"], fields[-3:]
    # ctypes: the member directly after mat_prec, four bytes, the last of the struct (bound by offset: tests/test_mat_prec_cpu.py pins
    # mat_prec as the last entry of _fields_)
    jp, mp = _lib.amgx_level_desc.jacobi_prec, _lib.amgx_level_desc.mat_prec
    assert jp.offset == mp.offset + mp.size and jp.size == 4 and jp.offset + jp.size == C.sizeof(_lib.amgx_level_desc)
    arr = (_lib.amgx_level_desc * 2)()
    assert arr[1].jacobi_prec == 0
    arr[1].jacobi_prec = 2
    arr[1].mat_prec = 1
    raw = bytes(arr)[C.sizeof(_lib.amgx_level_desc) + mp.offset:]
    assert raw[:8] == (1).to_bytes(4, "little") + (2).to_bytes(4, "little") and arr[0].jacobi_prec == 0 and arr[1].jacobi_prec == 2
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "amgx.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(amgx_level_desc), offsetof(amgx_level_desc, jacobi_prec),'
                   ' offsetof(amgx_level_desc, mat_prec));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off, off_mp = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.amgx_level_desc)
    assert off == _lib.amgx_level_desc.jacobi_prec.offset and off_mp == _lib.amgx_level_desc.mat_prec.offset


def test_enum_and_query_are_declared(tmp_path):
    from ngsamg_amd import _lib
    h = " ".join(_header().split())
    assert "enum { AMGX_JACOBI_PREC_F64 = 0, AMGX_JACOBI_PREC_F32 = 1, AMGX_JACOBI_PREC_F32_WIDE = 2 };" in h
    assert "int amgx_jacobi_prec_info(amgx_handle h, int level, int64_t* out, int n_out);" in h
    assert "#define AMGX_JACOBI_PREC_INFO_N 5" in h
    assert (_lib.AMGX_JACOBI_PREC_F64, _lib.AMGX_JACOBI_PREC_F32, _lib.AMGX_JACOBI_PREC_F32_WIDE) == (0, 1, 2)
    assert "amgx_jacobi_prec_info" in _lib.AMGX_SYMBOLS
    # what existing interfaces pin stays: the entry counts and the strings of mat_prec
    assert "#define AMGX_LEVEL_EXTRA_N 12" in h and "enum { AMGX_PREC_F64 = 0, AMGX_PREC_F32 = 1 };" in h
    src, exe = tmp_path / "en.c", tmp_path / "en"
    src.write_text('#include <stdio.h>\n#include "amgx.h"\nint main(void){int (*q)(amgx_handle, int, int64_t*, int) = amgx_jacobi_prec_info;'
                   ' (void)q; printf("%d %d %d\\n", AMGX_JACOBI_PREC_F64, AMGX_JACOBI_PREC_F32, AMGX_JACOBI_PREC_F32_WIDE);return 0;}\n')
    subprocess.check_call(["gcc", "-c", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])


def test_vocabulary_of_jacobi_prec():
    from ngsamg_amd._lib import NgsAMGError as E
    from ngsamg_amd.device import jacobi_prec_levels as jp
    assert jp("single", ["jacobi"] * 4) == [1, 1, 1, 0]
    assert jp("single_wide", ["jacobi"] * 3) == [2, 2, 0]
    assert jp("double", ["jacobi"] * 3) == [0, 0, 0]
    assert jp("single", ["jacobi"]) == [1]                                          # a stand-alone smoother is smoothed
    assert jp("single", ["jacobi", "cheby", "hgs", "jacobi"]) == [1, 0, 0, 0]       # a scalar request: the scalar Jacobi levels
    assert jp("single", ["jacobi", "jacobi", "jacobi"], [3, 1, 1]) == [0, 1, 0]     # ... block Jacobi levels are not among them
    assert jp(["single", "double", "single_wide", "double"], ["jacobi"] * 4) == [1, 0, 2, 0]
    assert jp(["double", "double", "single"], ["cheby", "jacobi", "jacobi"]) == [0, 0, 0]     # the coarsest ignores the field
    with pytest.raises(E, match="no scalar Jacobi level"):
        jp("single", ["cheby", "hgs", "jacobi"])
    with pytest.raises(E, match="no scalar Jacobi level"):
        jp("single_wide", ["jacobi", "jacobi"], [3, 6])
    with pytest.raises(E, match="level 1.*scalar Jacobi levels only.*cheby"):
        jp(["double", "single", "double"], ["jacobi", "cheby", "jacobi"])
    with pytest.raises(E, match="level 0.*block size 3"):
        jp(["single", "double"], ["jacobi", "jacobi"], [3, 6])
    with pytest.raises(E, match="one entry per level"):
        jp(["single"], ["jacobi", "jacobi"])
    for bad in ("float", "single_gs", 1, None, ["single", "half"]):
        with pytest.raises(E, match="unknown jacobi_prec"):
            jp(bad, ["jacobi", "jacobi"])


def test_descriptor_carries_the_field_and_leaves_mat_prec():
    from ngsamg_amd.device import hierarchy_desc
    p, H = poisson_case(*PROBLEMS[1])
    n = H.n_levels
    assert n >= 3
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi", jacobi_prec="single")
    assert [desc.levels[i].jacobi_prec for i in range(n)] == [1] * (n - 1) + [0]
    assert [desc.levels[i].mat_prec for i in range(n)] == [0] * n
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi")
    assert [desc.levels[i].jacobi_prec for i in range(n)] == [0] * n
    per = ["single_wide"] + ["double"] * (n - 2) + ["single"]
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi", jacobi_prec=per)
    assert [desc.levels[i].jacobi_prec for i in range(n)] == [2] + [0] * (n - 1)
    # both options on one hierarchy: Jacobi on level 0, Chebyshev below
    types = ["jacobi"] + ["cheby"] * (n - 1)
    desc, keep, _ = hierarchy_desc(H, sm_type=types, mat_prec="single", jacobi_prec="single")
    assert [desc.levels[i].jacobi_prec for i in range(n)] == [1] + [0] * (n - 1)
    assert [desc.levels[i].mat_prec for i in range(n)] == [0] + [1] * (n - 2) + [0]


def test_python_errors_come_before_the_library(monkeypatch):
    import inspect
    import ngsamg_amd.NgsAMG as N
    from ngsamg_amd import _lib
    from ngsamg_amd.device import DeviceAMGMatrix
    from ngsamg_amd.dist import DistributedAMG

    def no_lib():
        raise AssertionError("the library was loaded")

    p, H = poisson_case(*PROBLEMS[1])
    pe, He = elasticity_case((7, 6, 5), False, 5)
    monkeypatch.setattr(_lib, "hip", no_lib)
    with pytest.raises(N.NgsAMGError, match="no scalar Jacobi level"):
        DeviceAMGMatrix(H, sm_type="cheby", jacobi_prec="single")
    with pytest.raises(N.NgsAMGError, match="unknown jacobi_prec"):
        DeviceAMGMatrix(H, sm_type="jacobi", jacobi_prec="half")
    with pytest.raises(N.NgsAMGError, match="level 0.*scalar Jacobi levels only"):
        DeviceAMGMatrix(H, sm_type="hgs", jacobi_prec=["single"] + ["double"] * (H.n_levels - 1))
    with pytest.raises(N.NgsAMGError, match="no scalar Jacobi level"):
        DeviceAMGMatrix(He, sm_type="jacobi", jacobi_prec="single")              # block Jacobi levels only
    with pytest.raises(N.NgsAMGError, match="rank-partitioned"):
        DistributedAMG(None, [], jacobi_prec="single")
    monkeypatch.undo()                   # (the host setup of Preconditioner may load the library for its Galerkin products)
    # the preconditioner flag (the Probe technique of tests/test_mat_prec_gs_cpu.py)
    seen = {}

    class Probe:
        def __init__(self, hier, **kw):
            seen.clear()
            seen.update(kw, hier=hier)
            raise N.NgsAMGError("probe")

    monkeypatch.setattr(N, "DeviceAMGMatrix", Probe)
    for flags, want in ((dict(ngs_amg_jacobi_prec="single"), "single"), (dict(ngs_amg_jacobi_prec="Single_Wide"), "single_wide"),
                        (dict(ngs_amg_jacobi_prec=["Single", "double"]), ["single", "double"]), (dict(), "double")):
        with pytest.raises(N.NgsAMGError, match="probe"):
            N.Preconditioner(to_matrix(p), "ngs_amg.h1_scal", p.free, coords=p.coords, ngs_amg_max_coarse_size=10,
                             ngs_amg_sm_type="jacobi", **flags)
        assert seen["jacobi_prec"] == want and seen["mat_prec"] == "double", (flags, seen)
    with pytest.raises(N.NgsAMGError, match="probe"):
        N.CreateJacobiSmoother(to_matrix(p), p.free, jacobi_prec="single")
    assert seen["jacobi_prec"] == "single"
    monkeypatch.undo()
    with pytest.raises(N.NgsAMGError, match="no scalar Jacobi level"):
        N.Preconditioner(to_matrix(p), "ngs_amg.h1_scal", p.free, coords=p.coords, ngs_amg_max_coarse_size=10,
                         ngs_amg_sm_type="gs", ngs_amg_jacobi_prec="single")
    assert inspect.signature(N.CreateJacobiSmoother).parameters["jacobi_prec"].default == "double"
    assert inspect.signature(DeviceAMGMatrix.__init__).parameters["jacobi_prec"].default == "double"
    assert hasattr(DeviceAMGMatrix, "jacobi_prec_info")


# ---- 2. the numerics of the definition --------------------------------------------------------------------------------------
def test_fp64_emulation_is_the_oracle_cycle():
    """round32=False: the folded form is the literal Jacobi V(1,1) cycle of the oracle up to the order of additions"""
    from oracle.pyoracle import Oracle
    shape, diri, mcs = PROBLEMS[1]
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 1)
    ref = Oracle(H.levels, sm_type="jacobi").apply(np.array(b))
    for form in ("apre", "apre_wd", "dia", "double"):
        x = FoldedJacobiRef(H, round32=False, forms=[form] + ["apre"] * (H.n_levels - 2)).apply(b)
        assert np.linalg.norm(x - ref) <= 1e-13 * np.linalg.norm(ref), form


@pytest.mark.parametrize("shape,diri,mcs", PROBLEMS)
def test_rounding_the_images_as_stored(shape, diri, mcs):
    p, H = poisson_case(shape, diri, mcs)
    b = rhs(p, 1)
    A = H.levels[0].A.to_scipy()
    c64 = FoldedJacobiRef(H, round32=False)
    x64 = c64.apply(b)
    _, it64, e64 = pcg(c64, A, b, tol=1e-8, maxit=100)
    s64 = symmetry_defect(c64, b.size)
    for form in ("apre", "apre_wd", "dia"):
        below = "apre_wd" if form == "apre_wd" else "apre"
        c32 = FoldedJacobiRef(H, round32=True, forms=[form] + [below] * (H.n_levels - 2))
        change = np.linalg.norm(c32.apply(b) - x64) / np.linalg.norm(x64)
        _, it32, e32 = pcg(c32, A, b, tol=1e-8, maxit=100)
        s32 = symmetry_defect(c32, b.size)
        print(f"{shape} {form}: change {change:.2e} | pcg {it64} / {it32} | symmetry defect {s64:.1e} / {s32:.1e}")
        assert 1e-10 <= change <= CHANGE_MAX, (shape, form, change)
        assert it32 == it64, (shape, form, it64, it32)                   # the problems kept for the GPU test
        assert e32[-1] <= 1e-8 * e32[0] and e64[-1] <= 1e-8 * e64[0]
        assert s64 <= 1e-14 and s32 <= 1e-6, (s64, s32)
