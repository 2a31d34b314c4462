"""The fused down kernels (row product + ChunkRestrict: dia, sell, sell-win, sell-lw and the residual forms of the block-hybrid
Gauss-Seidel down pass) under the switches that every one of them carries a branch for and no other test sets:

  AMGX_RSUM_SORT=1                        the `dest` branch: partial sums stored row by row.  The partial sums are the same and every
                                          lane of restrict_sum_kernel adds them in the same order, so the result is bit for bit the
                                          default one.
  AMGX_NO_EP_NT=1 AMGX_NO_EP_HOIST=1      plain instead of non-temporal own-row loads / stores, operands loaded after the row product:
                                          the same operands in the same arithmetic, bit for bit the default result.
  AMGX_NO_WDIAG=1 (sell), AMGX_NO_FOLD=1  other arithmetic: against the oracle at the suite's bounds (1e-12 Jacobi, 1e-10 hgs).

Every case asserts through DeviceAMGMatrix.level_paths that its kernel ran -- "kernel" for the Jacobi cases, "gs_down" (the form of
gsb_residual_restrict) for sm_type="hgs" -- in the default run and under every switch.  In the hgs cases only AMGX_RSUM_SORT reaches
the down kernel itself: MODE 1 is launched without the nt flags and has no fold term, so the other switches there check the rest of
the cycle around it, not a branch of the family.  All three forms of the Gauss-Seidel down
pass are reachable on the 41 x 37 x 29 problem: sell and sell-win on level 0 with one lane per row (without or with length-sorted
windows), sell-lw on level 1 (its rows have the 24 entries that form asks for) with the lowered row threshold.
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


# name: (problem, sm_type, environment, level, expected entries of level_paths)
CASES = {
    "dia-ept4": (lambda: _fd7((2, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), 0, {"kernel": "dia", "ept": 4}),
    "dia-ept6": (lambda: _fd7((5, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), 0, {"kernel": "dia", "ept": 6}),
    "sell-g1-ept4": (lambda: _fd7((2, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_NO_DIA", "1"), ("AMGX_SELL_MAX_LANES", "1")), 0,
                     {"kernel": "sell", "lanes": 1, "ept": 4}),
    "sell-g1-ept6": (lambda: _fd7((5, 2)), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_NO_DIA", "1"), ("AMGX_SELL_MAX_LANES", "1")), 0,
                     {"kernel": "sell", "lanes": 1, "ept": 6}),
    "sell-g4": (_chain12, "jacobi", (("AMGX_SELL_MAX_LANES", "4"), ("AMGX_NO_LW", "1")), 0, {"kernel": "sell", "lanes": 4, "ept": 4}),
    # (one lane per row: with the 8 lanes this small level would get, amgx_create builds no windowed image)
    "sell-win": (_p3, "jacobi", (("AMGX_APRE_WINDOW", "1"), ("AMGX_NO_DENSE_TAIL", "1"), ("AMGX_SELL_MAX_LANES", "1")), 1, {"kernel": "sell-win"}),
    "sell-lw": (_p3, "jacobi", (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")), 1, {"kernel": "sell-lw"}),
    "hgs-sell": (_p3, "hgs", (("AMGX_SELL_MAX_LANES", "1"), ("AMGX_NO_SELL_WINDOW", "1"), ("AMGX_NO_DENSE_TAIL", "1")), 0,
                 {"gs_form": "hybrid", "gs_down": "sell"}),
    "hgs-sell-win": (_p3, "hgs", (("AMGX_SELL_MAX_LANES", "1"), ("AMGX_NO_DENSE_TAIL", "1")), 0, {"gs_form": "hybrid", "gs_down": "sell-win"}),
    "hgs-sell-lw": (_p3, "hgs", (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")), 1, {"gs_form": "hybrid", "gs_down": "sell-lw"}),
}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, monkeypatch, env, sm_type):
    from ngsamg_amd.device import DeviceAMGMatrix
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type=sm_type)


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
        else:
            _REF[key] = Oracle(H.levels, sm_type="jacobi").apply(b)
    return _REF[key]


@pytest.mark.parametrize("name", list(CASES))
def test_down_kernel_switches(name, monkeypatch):
    problem, sm_type, env, level, expect = CASES[name]
    H, b = problem()
    tol = 1e-12 if sm_type == "jacobi" else 1e-10

    def run(extra):
        dev = _dev(H, monkeypatch, env + extra, sm_type)
        lp = dev.level_paths(level)
        assert {k: lp[k] for k in expect} == expect, (extra, lp)
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
