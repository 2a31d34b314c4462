"""Single-precision images for Gauss-Seidel on SCALAR levels (mat_prec = "single_gs_all", AMGX_PREC_F32_SCALAR_GS)
without a GPU: the vocabulary of mat_prec and the descriptor values, the header, the one new fact of the multi-vector fusion rule
(multi_rule.hpp compiled with g++), and the numerics of the definition on the CPU -- the oracle in the device's sweep order on levels
whose A.val went through float32 (tests/mat_prec_ref.rounded_levels) with the dinv of the TRUE A, against the same oracle on the
hierarchy; the Krylov operator is the fp64 A in both.

Bounds (those of tests/test_mat_prec_gs_cpu.py): the relative change of one application in [1e-9, 1e-6] -- measured when the option
was proposed: 2.9e-8 ... 1.29e-7 over the five grids x two orders below, the largest at (33, 33) multicolour; the lower end shows that
the rounding is applied at all --, PCG iterations to 1e-8 equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.mat_prec_ref import pcg, rounded_levels
from tests.problems import elasticity_case, poisson_case, rhs, to_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(17, 17, 17), (33, 33), (40, 36), (24, 22, 20), (9, 9, 9)]


def _case(grid):
    return poisson_case(grid, "right|top", 20) if len(grid) == 3 else poisson_case(grid, "left|top", 5)


def _header():
    with open(os.path.join(ROOT, "include", "amgx.h")) as f:
        return f.read()


# ---- 1. the vocabulary and the descriptor ----------------------------------------------------------------------------------------
def test_single_gs_all_vocabulary():
    from ngsamg_amd import _lib
    from ngsamg_amd.device import mat_prec_levels
    E = _lib.NgsAMGError
    assert (_lib.AMGX_PREC_F64, _lib.AMGX_PREC_F32, _lib.AMGX_PREC_F32_SCALAR_GS) == (0, 1, 2)
    # 2 on the Gauss-Seidel levels, 1 on the Chebyshev levels, never the coarsest
    assert mat_prec_levels("single_gs_all", ["hgs"] * 4) == [2, 2, 2, 0]
    assert mat_prec_levels("single_gs_all", ["gs", "cheby", "jacobi", "gs"]) == [2, 1, 0, 0]
    assert mat_prec_levels("single_gs_all", ["hgs", "bgs", "cheby", "cheby"]) == [2, 0, 1, 0]
    assert mat_prec_levels("single_gs_all", ["gs"]) == [2]                              # a stand-alone smoother is smoothed
    assert mat_prec_levels("single_gs_all", ["cheby"] * 3) == mat_prec_levels("single", ["cheby"] * 3) == [1, 1, 0]
    # "single_gs" and "single" keep every value
    assert mat_prec_levels("single_gs", ["hgs"] * 4) == [1, 1, 1, 0]
    assert mat_prec_levels("single_gs", ["gs", "cheby", "jacobi", "gs"]) == [1, 1, 0, 0]
    assert mat_prec_levels("single", ["hgs", "cheby", "gs"]) == [0, 1, 0]
    assert mat_prec_levels("double", ["hgs"] * 3) == [0, 0, 0]
    # as a scalar it needs at least one such level
    for types in (["jacobi"] * 3, ["bgs", "jacobi", "gs"], ["jacobi", "jacobi", "hgs"]):       # (gs on the coarsest only)
        with pytest.raises(E, match="single_gs_all.*no Chebyshev or Gauss-Seidel level"):
            mat_prec_levels("single_gs_all", types)
        with pytest.raises(E, match="'single_gs'.*no Chebyshev or Gauss-Seidel level"):
            mat_prec_levels("single_gs", types)
    # per-level lists: on those levels only, the coarsest ignores its entry
    assert mat_prec_levels(["single_gs_all", "double", "single_gs_all"], ["hgs", "hgs", "jacobi"]) == [2, 0, 0]
    assert mat_prec_levels(["single_gs_all", "single_gs", "single", "double"], ["gs", "hgs", "cheby", "gs"]) == [2, 1, 1, 0]
    assert mat_prec_levels(["double", "single_gs_all", "single_gs_all"], ["jacobi", "cheby", "bgs"]) == [0, 1, 0]
    for bad_type in ("jacobi", "bgs"):
        with pytest.raises(E, match="'single_gs_all' on level 1.*" + bad_type):
            mat_prec_levels(["double", "single_gs_all", "double"], ["hgs", bad_type, "hgs"])
        with pytest.raises(E, match="'single_gs' on level 1.*" + bad_type):
            mat_prec_levels(["double", "single_gs", "double"], ["hgs", bad_type, "hgs"])
    for bad in ("single-gs-all", "SINGLE_GS_ALL", "single_hgs", "single_all", 2, None, ["single_gs_all", "half"]):
        with pytest.raises(E, match="unknown mat_prec"):
            mat_prec_levels(bad, ["hgs", "hgs"])


def test_descriptor_of_scalar_and_block_levels():
    """scalar Gauss-Seidel levels carry AMGX_PREC_F32_SCALAR_GS under "single_gs_all" and 0 under "single_gs"; block levels
    AMGX_PREC_F32 under both"""
    from ngsamg_amd.device import hierarchy_desc
    ps, Hs = poisson_case((33, 33), "left|top", 5)
    n = Hs.n_levels
    for sm in ("hgs", "gs"):
        desc, keep, _ = hierarchy_desc(Hs, sm_type=sm, mat_prec="single_gs_all")
        assert [desc.levels[i].mat_prec for i in range(n)] == [2] * (n - 1) + [0], sm
        desc, keep, _ = hierarchy_desc(Hs, sm_type=sm, mat_prec="single_gs")
        assert [desc.levels[i].mat_prec for i in range(n)] == [0] * n, sm              # still the double handle
        desc, keep, _ = hierarchy_desc(Hs, sm_type=sm)
        assert [desc.levels[i].mat_prec for i in range(n)] == [0] * n, sm
    tys = ["gs", "cheby"] + ["hgs"] * (n - 2)
    desc, keep, _ = hierarchy_desc(Hs, sm_type=tys, mat_prec="single_gs_all")
    assert [desc.levels[i].mat_prec for i in range(n)] == [2, 1] + [2] * (n - 3) + [0]
    desc, keep, _ = hierarchy_desc(Hs, sm_type=tys, mat_prec=["single_gs_all", "double"] + ["single_gs"] * (n - 2))
    assert [desc.levels[i].mat_prec for i in range(n)] == [2] + [0] * (n - 1)
    # a block hierarchy: "single_gs_all" is "single_gs"
    pb, Hb = elasticity_case((7, 6, 5), False, 5)
    nb = Hb.n_levels
    for sm in ("hgs", "gs"):
        a = hierarchy_desc(Hb, sm_type=sm, mat_prec="single_gs_all")
        b = hierarchy_desc(Hb, sm_type=sm, mat_prec="single_gs")
        assert [a[0].levels[i].mat_prec for i in range(nb)] == [b[0].levels[i].mat_prec for i in range(nb)] == [1] * (nb - 1) + [0], sm


def test_preconditioner_flag_standalone_smoother_and_dist():
    import inspect
    import ngsamg_amd.NgsAMG as N
    from ngsamg_amd.device import DeviceAMGMatrix
    seen = {}

    class Probe:
        def __init__(self, hier, **kw):
            seen.clear()
            seen.update(kw, hier=hier)
            raise N.NgsAMGError("probe")

    p, H = poisson_case((9, 9), "left|top", 5)
    old = N.DeviceAMGMatrix
    N.DeviceAMGMatrix = Probe
    try:
        for flags, want in ((dict(ngs_amg_sm_type="hgs", ngs_amg_mat_prec="single_gs_all"), "single_gs_all"),
                            (dict(ngs_amg_sm_type="gs", ngs_amg_mat_prec="Single_GS_All"), "single_gs_all"),
                            (dict(ngs_amg_sm_type="hgs"), "double")):
            with pytest.raises(N.NgsAMGError, match="probe"):
                N.Preconditioner(to_matrix(p), "ngs_amg.h1_scal", p.free, coords=p.coords, ngs_amg_dim=2, ngs_amg_max_coarse_size=5, **flags)
            assert seen["mat_prec"] == want, (flags, seen["mat_prec"])
    finally:
        N.DeviceAMGMatrix = old
    # a request that cannot be met is refused before the library is loaded
    with pytest.raises(N.NgsAMGError, match="single_gs_all.*no Chebyshev or Gauss-Seidel level"):
        DeviceAMGMatrix(H, sm_type="jacobi", mat_prec="single_gs_all")
    assert inspect.signature(N.CreateHybridGSS).parameters["mat_prec"].default == "double"
    assert hasattr(DeviceAMGMatrix, "gs_prec_info")
    assert DeviceAMGMatrix._GSPREC_IMAGES == ("A", "full", "fullLW", "lowin", "rest", "restLW", "sell", "lower", "upper")
    assert len(DeviceAMGMatrix._EXTRA_KEYS) == 12
    # rank-partitioned hierarchies refuse it before the library is called
    from ngsamg_amd.dist import DistributedAMG
    for mp in ("single_gs_all", ["Single_GS_All", "double"]):
        with pytest.raises(N.NgsAMGError, match="single_gs_all.*rank-partitioned"):
            DistributedAMG(None, [], sm_type="hgs", mat_prec=mp)


# ---- 2. the header --------------------------------------------------------------------------------------------------------------
def test_header_enum_query_and_struct_size(tmp_path):
    from ngsamg_amd import _lib
    raw = _header()
    lines = raw.splitlines()
    pinned = "enum { AMGX_PREC_F64 = 0, AMGX_PREC_F32 = 1 };"
    i = next(k for k, ln in enumerate(lines) if ln.startswith(pinned))
    assert lines[i + 1] == "enum { AMGX_PREC_F32_SCALAR_GS = 2 }; /* amgx_level_desc.mat_prec, scalar AMGX_SM_GS levels only */", lines[i + 1]
    h = " ".join(raw.split())
    assert "#define AMGX_LEVEL_EXTRA_N 12" in h and "#define AMGX_JACOBI_PREC_INFO_N 5" in h and "#define AMGX_GS_PREC_INFO_N 5" in h
    assert "int amgx_gs_prec_info(amgx_handle h, int level, int64_t* out, int n_out);" in h
    assert "amgx_gs_prec_info" in _lib.AMGX_SYMBOLS and _lib.AMGX_GS_PREC_INFO_N == 5
    for word in ("AMGX_PREC_F32_SCALAR_GS", "AMGX_GS_F32_WIDE", "AMGX_NO_MAT_F32", "rank-partitioned"):
        assert word in h
    assert "single-precision Gauss-Seidel images (level l)" in h.replace("* ", "")
    # the struct: mat_prec stays the last entry of _fields_, jacobi_prec ends the struct, sizeof as gcc sees it
    assert _lib.amgx_level_desc._fields_[-1][0] == "mat_prec"
    jp = _lib.amgx_level_desc.jacobi_prec
    assert jp.offset + jp.size == C.sizeof(_lib.amgx_level_desc)
    src, exe = tmp_path / "sz.c", tmp_path / "sz"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "amgx.h"\n'
                   'int main(void){int (*q)(amgx_handle, int, int64_t*, int) = amgx_gs_prec_info; (void)q;'
                   'printf("%zu %zu %d %d\\n", sizeof(amgx_level_desc), offsetof(amgx_level_desc, jacobi_prec) + sizeof(int32_t),'
                   ' AMGX_PREC_F32_SCALAR_GS, AMGX_GS_PREC_INFO_N);return 0;}\n')
    subprocess.check_call(["gcc", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz.o"), str(src)])
    src2 = tmp_path / "sz2.c"
    src2.write_text(src.read_text().replace("int (*q)(amgx_handle, int, int64_t*, int) = amgx_gs_prec_info; (void)q;", ""))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src2)])
    size, end, value, n_info = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == end == C.sizeof(_lib.amgx_level_desc) and value == 2 and n_info == 5


# ---- 3. the fusion rule -----------------------------------------------------------------------------------------------------------
RULE_PROGRAM = r"""
#include "multi_rule.hpp"
#include <cstdio>
#include <cstring>
using namespace amgx;
using F = MultiLevelFacts;

// multi_level_reason as it was before the fact sgs_f32 existed
static const char* parent_reason(int rule, const F& f) {
  const bool base = rule == 0;
  const bool jacobi = f.sm_type == AMGX_SM_JACOBI, cheby = f.sm_type == AMGX_SM_CHEBY;
  const bool gs = f.smoothed && rule >= 2 && f.sm_type == AMGX_SM_GS;
  auto smoother = [&]() -> const char* {
    if (!f.smoothed) return nullptr;
    if (rule >= 2 && f.sm_type == AMGX_SM_BGS) return "block Gauss-Seidel (bgs) smoother";
    if (rule == 2 && gs && f.bs != 1) return "Gauss-Seidel on a block level";
    if (!(jacobi || (cheby && !base) || gs))
      return base ? "smoother is not Jacobi" : rule == 1 ? "smoother is not Jacobi or Chebyshev" : "smoother is not Jacobi, Chebyshev or Gauss-Seidel";
    if (!f.plain) return "sm_steps > 1 or sm_symm";
    if (cheby && (f.cheb_degree < 1 || f.cheb_degree > 8)) return "Chebyshev level without coefficients";
    return nullptr;
  };
  auto level = [&]() -> const char* {
    if (base && f.bs != 1) return "block level";
    if (f.bs != 1 && f.bs != 2 && f.bs != 3 && f.bs != 6) return "block size is not 1, 2, 3 or 6";
    if (!f.square) return "ghost columns";
    if (f.permuted) return "renumbered level";
    if (f.jacobi_f32) return "single-precision Jacobi images";
    if (gs && !f.empty) {
      if (rule >= 3 && f.gs_f32) return "single-precision Gauss-Seidel images";
      if (!(f.bs == 1 ? f.sweep_ok : f.block_sweep_ok)) return "Gauss-Seidel sweep form without a multi-vector kernel";
      if (f.bs != 1 && !f.block_sweep_fits) return "sweep block too large for the multi-vector sweep";
    }
    if (!f.empty && !(base ? f.a_scalar : f.a_level)) return "level matrix format";
    return nullptr;
  };
  const char* why = base ? level() : smoother();
  if (!why) why = base ? smoother() : level();
  if (!why && f.smoothed && !f.empty && !(base ? f.t_scalar : f.t_transfer)) why = "transfer format";
  return why;
}
static bool same(const char* a, const char* b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

int main() {
  if (F().sgs_f32) { std::printf("the fact does not default to false\n"); return 1; }
  // with the fact false every decision is the parent's
  long n = 0;
  for (int bs : {1, 2, 3, 4, 6}) for (int sm = 0; sm < 4; ++sm) for (int deg : {0, 2, 9}) for (int bits = 0; bits < (1 << 14); ++bits) {
    F f;
    f.bs = bs; f.sm_type = sm; f.cheb_degree = deg;
    f.smoothed = bits & 1; f.plain = bits & 2; f.empty = bits & 4; f.square = bits & 8; f.permuted = bits & 16; f.jacobi_f32 = bits & 32; f.gs_f32 = bits & 64;
    f.a_scalar = bits & 128; f.a_level = bits & 256; f.t_scalar = bits & 512; f.t_transfer = bits & 1024;
    f.sweep_ok = bits & 2048; f.block_sweep_ok = bits & 4096; f.block_sweep_fits = bits & 8192;
    for (int rule = 0; rule < 4; ++rule, ++n)
      if (!same(multi_level_reason(rule, f), parent_reason(rule, f))) { std::printf("rule %d differs from the parent's (bs %d sm %d bits %d)\n", rule, bs, sm, bits); return 1; }
  }
  // the fact: a scalar Gauss-Seidel level that every rule from 2 on would admit keeps the column loop, whether the sweep form has kernels or not
  for (int sweep_ok = 0; sweep_ok < 2; ++sweep_ok) {
    F lev[2];
    for (F& f : lev) { f.a_scalar = f.a_level = f.t_scalar = f.t_transfer = true; f.sm_type = AMGX_SM_GS; f.sweep_ok = true; }
    lev[0].smoothed = true;
    for (int rule = 2; rule < 4; ++rule) if (multi_handle_rule(rule, true, lev, 2).fused != 1) { std::printf("the double handle is not fused under rule %d\n", rule); return 1; }
    lev[0].sgs_f32 = true; lev[0].sweep_ok = sweep_ok;
    for (int rule = 2; rule < 4; ++rule) {
      const MultiDecision d = multi_handle_rule(rule, true, lev, 2);
      if (d.fused != 0 || d.why != "single-precision Gauss-Seidel images (level 0)") { std::printf("rule %d: '%s'\n", rule, d.why.c_str()); return 1; }
    }
    // rules 0 and 1 never admitted a Gauss-Seidel level: their answer stays
    for (int rule = 0; rule < 2; ++rule) if (!same(multi_level_reason(rule, lev[0]), parent_reason(rule, lev[0]))) { std::printf("rule %d changed\n", rule); return 1; }
  }
  std::printf("ok %ld\n", n);
  return 0;
}
"""


def test_fusion_rule_has_one_new_fact(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile multi_rule.hpp")
    src, exe = tmp_path / "rule.cpp", tmp_path / "rule"
    src.write_text(RULE_PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ngsamg_amd", "csrc", "device"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ---- 4. the numerics of the definition --------------------------------------------------------------------------------------------
ORDERS = {"block-hybrid": "hgs", "multicolour": "gs"}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("grid", GRIDS, ids=["x".join(map(str, g)) for g in GRIDS])
def test_rounding_the_images_costs_nothing(grid, order):
    """the oracle in the device's sweep order; A.val of every smoothed level through float32, dinv that of the true A"""
    from ngsamg_amd.device import hierarchy_desc
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    p, H = _case(grid)
    sm = ORDERS[order]
    smoothed = list(range(H.n_levels - 1))
    R = rounded_levels(H, smoothed)
    assert not np.array_equal(np.asarray(R[0].A.val), np.asarray(H.levels[0].A.val)) and R[0].dinv is H.levels[0].dinv
    if sm == "hgs":
        _, _, info = hierarchy_desc(H, sm_type="hgs")       # blocks, colours and dinv of the TRUE A
        assert info[0] is not None
        lv64, types = hgs_levels(H.levels, info)
        lv32, types32 = hgs_levels(R, info)
        assert types == types32 and types[0] == "gs_order"
    else:
        lv64, lv32, types = H.levels, R, "gs_mc"
    o64, o32 = Oracle(lv64, sm_type=types), Oracle(lv32, sm_type=types)
    b = rhs(p, 3)
    x64, x32 = o64.apply(np.array(b)), o32.apply(np.array(b))
    change = np.linalg.norm(x32 - x64) / np.linalg.norm(x64)
    A = H.levels[0].A.to_scipy()
    _, it64, e64 = pcg(o64, A, b, tol=1e-8, maxit=100)
    _, it32, e32 = pcg(o32, A, b, tol=1e-8, maxit=100)
    print(f"{grid} {order}: change {change:.2e} | pcg {it64} / {it32}")
    assert 1e-9 <= change <= 1e-6, (grid, order, change)
    assert it64 == it32, (grid, order, it64, it32)
    assert e32[-1] <= 1e-8 * e32[0] and e64[-1] <= 1e-8 * e64[0]
