"""The fused down kernels (row product + ChunkRestrict: dia, sell, sell-win, sell-lw and the residual forms of the block-hybrid
Gauss-Seidel down pass) under the switches that every one of them carries a branch for and no other test sets:

  AMGX_RSUM_SORT=1                        the `dest` branch: partial sums stored row by row.  The partial sums are the same and every
                                          lane of restrict_sum_kernel adds them in the same order, so the result is bit for bit the
                                          default one.
  AMGX_NO_EP_NT=1 AMGX_NO_EP_HOIST=1      plain instead of non-temporal own-row loads / stores, operands loaded after the row product:
                                          the same operands in the same arithmetic, bit for bit the default result.
  AMGX_NO_WDIAG=1 (sell), AMGX_NO_FOLD=1  other arithmetic: against the reference at the suite's bounds (1e-12 Jacobi and
                                          Chebyshev, 1e-10 hgs).

Every case asserts through DeviceAMGMatrix.level_paths that its kernel ran -- "kernel" for the Jacobi and Chebyshev cases, "gs_down"
(the form of gsb_residual_restrict) for sm_type="hgs" -- in the default run and under every switch, with the workgroup size, the
lanes per row and the entries of P per thread where the launcher has an instantiation per value (the table of DESIGN.md 5.2).
The Chebyshev cases (MODE 2, degree 2 on given interval ends) are checked against tests/cheby_ref.py at 1e-12; "cheby-f32" is the
same with mat_prec="single": the kernel reads the float image (matrix_info "A32"), and the reference is computed on the matrices
rounded to single precision on the levels that have one (tests/mat_prec_ref.py), which that handle reproduces bit for bit
(test_gpu_mat_prec.py), so the bound is the same 1e-12.

In the hgs cases only AMGX_RSUM_SORT reaches the down kernel itself: MODE 1 is launched without the nt flags and has no fold term,
so the other switches there check the rest of the cycle around it, not a branch of the family.  All three forms of the
Gauss-Seidel down pass are reachable on the 41 x 37 x 29 problem: sell and sell-win on level 0 with one lane per row (without or
with length-sorted windows), sell-lw on level 1 (its rows have the 24 entries that form asks for) with the lowered row threshold.
Open gap: level_paths reports the form of the launch through RG ("gs_down") but neither its lanes nor its entries of P per thread,
so no test asserts which <EPT, G> of the MODE 1 kernels ran.
"""
import functools

import numpy as np
import pytest

from tests import reorder as R
from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

P3 = ((41, 37, 29), "right|top", 10)


@functools.lru_cache(maxsize=None)
def _hand(kind, shape, per_row):
    A, _ = R.stencil(kind, shape, seed=3)
    return R.hand_hierarchy(A, per_row=per_row, agg=8, seed=3), np.random.default_rng(3).standard_normal(A.shape[0])


def _fd7(per_row):
    return _hand("fd7", (41, 37, 29), per_row)


def _chain12():
    return _hand("offsets:" + ",".join(str(o) for o in range(1, 13)), (20000,), (2, 2))


def _p3():
    p, H = poisson_case(*P3)
    return H, rhs(p, 1)


@functools.lru_cache(maxsize=None)
def _p3_wide():
    """level 1 of the Kuhn problem (long rows) with a 5-entry prolongation below it: 1280 entries of P in a 256-row chunk"""
    p, H0 = poisson_case(*P3)
    H = R.hand_hierarchy(H0.levels[0].A.to_scipy(), per_row=(5, 2), agg=8, seed=5, first_P=(H0.levels[0].P.to_scipy(),))
    return H, np.random.default_rng(5).standard_normal(p.n)


# name: (problem, sm_type, environment, level, expected entries of level_paths)
ONE = (("AMGX_SELL_MAX_LANES", "1"),)
SELL_G1 = (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_NO_DIA", "1")) + ONE


def _lanes(g):
    return (("AMGX_SELL_MAX_LANES", str(g)),)


def _cheb(g, ept=4):
    return {"kernel": "cheby-res", "fused_block": 512, "lanes": g, "ept": ept}


CASES = {
    "dia-ept4": (lambda: _fd7((2, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), 0, {"kernel": "dia", "ept": 4}),
    "dia-ept6": (lambda: _fd7((5, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), 0, {"kernel": "dia", "ept": 6}),
    "sell-g1-ept4": (lambda: _fd7((2, 2)), "jacobi", SELL_G1, 0, {"kernel": "sell", "fused_block": 512, "lanes": 1, "ept": 4}),
    "sell-g1-ept6": (lambda: _fd7((5, 2)), "jacobi", SELL_G1, 0, {"kernel": "sell", "fused_block": 512, "lanes": 1, "ept": 6}),
    "sell-g1-ept4-fb256": (lambda: _fd7((2, 2)), "jacobi", SELL_G1 + (("AMGX_FUSED_BLOCK", "256"),), 0,
                           {"kernel": "sell", "fused_block": 256, "lanes": 1, "ept": 4}),
    "sell-g1-ept4-fb1024": (lambda: _fd7((2, 2)), "jacobi", SELL_G1 + (("AMGX_FUSED_BLOCK", "1024"),), 0,
                            {"kernel": "sell", "fused_block": 1024, "lanes": 1, "ept": 4}),
    "sell-g4": (_chain12, "jacobi", _lanes(4) + (("AMGX_NO_LW", "1"),), 0, {"kernel": "sell", "lanes": 4, "ept": 4}),
    # (one lane per row: with the 8 lanes this small level would get, amgx_create builds no windowed image)
    "sell-win": (_p3, "jacobi", (("AMGX_APRE_WINDOW", "1"), ("AMGX_NO_DENSE_TAIL", "1")) + ONE, 1, {"kernel": "sell-win", "lanes": 1, "ept": 4}),
    "sell-lw-ept4": (_p3_wide, "jacobi", (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")), 1, {"kernel": "sell-lw", "lanes": 2, "ept": 4}),
    "sell-lw": (_p3, "jacobi", (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")), 1, {"kernel": "sell-lw", "lanes": 2, "ept": 2}),
    # MODE 2: one lane with 4 / 6 entries of P per thread, 2 / 4 / 8 lanes; each on the fp64 and on the float image
    "cheby-g1-ept4": (lambda: _fd7((2, 2)), "cheby", ONE, 0, _cheb(1)),
    "cheby-g1-ept6": (lambda: _fd7((5, 2)), "cheby", ONE, 0, _cheb(1, 6)),
    "cheby-g2": (_chain12, "cheby", _lanes(2), 0, _cheb(2)),
    "cheby-g4": (_chain12, "cheby", _lanes(4), 0, _cheb(4)),
    "cheby-g8": (_chain12, "cheby", _lanes(8), 0, _cheb(8)),
    "cheby-f32-g1-ept4": (lambda: _fd7((2, 2)), "cheby-f32", ONE, 0, _cheb(1)),
    "cheby-f32-g1-ept6": (lambda: _fd7((5, 2)), "cheby-f32", ONE, 0, _cheb(1, 6)),
    "cheby-f32-g2": (_chain12, "cheby-f32", _lanes(2), 0, _cheb(2)),
    "cheby-f32-g4": (_chain12, "cheby-f32", _lanes(4), 0, _cheb(4)),
    "cheby-f32-g8": (_chain12, "cheby-f32", _lanes(8), 0, _cheb(8)),
    "hgs-sell": (_p3, "hgs", ONE + (("AMGX_NO_SELL_WINDOW", "1"), ("AMGX_NO_DENSE_TAIL", "1")), 0, {"gs_form": "hybrid", "gs_down": "sell"}),
    "hgs-sell-win": (_p3, "hgs", ONE + (("AMGX_NO_DENSE_TAIL", "1"),), 0, {"gs_form": "hybrid", "gs_down": "sell-win"}),
    "hgs-sell-lw": (_p3, "hgs", (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")), 1, {"gs_form": "hybrid", "gs_down": "sell-lw"}),
}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def _lmax(H):
    """interval ends of the Chebyshev case, different on every level"""
    from tests.cheby_ref import power_estimate
    return tuple(1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]) + (1.0,)


def _dev(H, monkeypatch, env, sm_type):
    from ngsamg_amd.device import DeviceAMGMatrix
    kw = {"cheb_lambda_max": list(_lmax(H))} if sm_type.startswith("cheby") else {}
    if sm_type == "cheby-f32":
        kw["mat_prec"] = "single"
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type=sm_type.split("-")[0], **kw)


_REF = {}


def _oracle(name, H, dev, sm_type, b):
    """the oracle's result, once per (hierarchy, smoother): none of the switches of this file changes what is computed"""
    from oracle.pyoracle import Oracle
    key = (id(H), sm_type) if sm_type == "jacobi" else (id(H), sm_type, CASES[name][2])     # (the hierarchies are cached: same object)
    if key not in _REF:
        if sm_type == "hgs":
            from tests.hgs_oracle import hgs_levels
            lv, types = hgs_levels(H.levels, dev.hgs)
            _REF[key] = Oracle(lv, sm_type=types).apply(b)
        elif sm_type.startswith("cheby"):
            from tests.cheby_ref import ChebyRef
            RH = H
            if sm_type == "cheby-f32":      # the levels whose smoother passes read the float image, rounded
                from tests.mat_prec_ref import RoundedHierarchy
                RH = RoundedHierarchy(H, [l for l in range(H.n_levels) if dev.matrix_info(l, "A32")["fmt"] is not None])
            _REF[key] = ChebyRef(RH, sm="cheby", degree=2, lambda_max=list(_lmax(H))).apply(b)
        else:
            _REF[key] = Oracle(H.levels, sm_type="jacobi").apply(b)
    return _REF[key]


@pytest.mark.parametrize("name", list(CASES))
def test_down_kernel_switches(name, monkeypatch):
    problem, sm_type, env, level, expect = CASES[name]
    H, b = problem()
    tol = 1e-10 if sm_type == "hgs" else 1e-12

    def run(extra):
        dev = _dev(H, monkeypatch, env + extra, sm_type)
        lp = dev.level_paths(level)
        assert {k: lp[k] for k in expect} == expect, (extra, lp)
        if sm_type.startswith("cheby"):     # which image MODE 2 reads
            a32 = dev.matrix_info(level, "A32")
            assert (a32["fmt"], a32["lanes"]) == ("sell", expect["lanes"]) if sm_type == "cheby-f32" else a32["fmt"] is None, a32
        x = np.full(b.size, np.nan)
        dev.Mult(b, x)
        return dev, x

    dev, x0 = run(())
    ref = _oracle(name, H, dev, sm_type, b)
    print(f"{name}: default vs oracle {_rel(x0, ref):.3e}")
    assert _rel(x0, ref) < tol
    _, x = run((("AMGX_RSUM_SORT", "1"),))
    assert np.array_equal(x, x0), "AMGX_RSUM_SORT"
    _, x = run((("AMGX_NO_EP_NT", "1"), ("AMGX_NO_EP_HOIST", "1")))
    assert np.array_equal(x, x0), "AMGX_NO_EP_NT AMGX_NO_EP_HOIST"
    others = (("AMGX_NO_WDIAG", "AMGX_NO_FOLD") if expect.get("kernel") == "sell" else ("AMGX_NO_FOLD",))
    for var in others:
        _, x = run(((var, "1"),))
        print(f"{name}: {var} vs oracle {_rel(x, ref):.3e}")
        assert _rel(x, ref) < tol, var
