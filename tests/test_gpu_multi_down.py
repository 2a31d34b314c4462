"""AMGX_MULTI_FUSE_DOWN (fuse="down" / "gs+down"): the fused down pass -- residual in LDS, chunk-local restriction --
of the multi-vector cycle.

Every test first asserts through level_paths and multi_level_plan that the level under test takes the kernel it means to test.

1. The stage (DownMulti) with the bit against the stage without it, array_equal per column: the multi-vector kernels read the same
   image, add in the same order per column, form the same slot sums and add the partial sums in the order of restrict_sum_kernel.
   The Chebyshev smooth from zero of a group runs the literal recurrence of the multi-vector cycle (diag + EP_CHEB products), which
   is the arithmetic of cheb_smooth but NOT bit-equal to it (measured: equal at degree 1, up to 3.3e-16 relative per column at degree 2), so the
   Chebyshev stage with x_given = 0 is held to the suite's bound for same-arithmetic comparisons, 1e-13 per column; with
   x_given = 1 (the down kernel alone) it is array_equal like every other case.
2. No column sees its neighbours: other widths, permuted neighbours, a NaN column.
3. The cycle (MultMulti) against the oracle (1e-12 Jacobi and Chebyshev, 1e-10 Gauss-Seidel in the GPU order), against
   Mult per column (1e-12), graph replay = direct launches = a fresh handle, a call without the bit afterwards = a handle that
   never saw the bit, k = 1 = Mult.
4. Levels that stay literal say why, and the bit changes nothing there.
5. PCG: iteration counts with and without the bit differ by one at most.
"""
import functools
import os

import numpy as np
import pytest

from tests import reorder as R
from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = (("AMGX_NO_DENSE_TAIL", "1"),)
ONE = (("AMGX_SELL_MAX_LANES", "1"),)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- problems (cached: the hierarchies are shared by the cases) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand(kind, shape, per_row, agg=8):
    A, _ = R.stencil(kind, shape, seed=3)
    return R.hand_hierarchy(A, per_row=per_row, agg=agg, seed=3)


def _fd7(per_row, agg=8):
    return _hand("fd7", (41, 37, 29), per_row, agg)


def _chain12():
    return _hand("offsets:" + ",".join(str(o) for o in range(1, 13)), (20000,), (2, 2))


@functools.lru_cache(maxsize=None)
def _poisson(shape, dirichlet="right|top", mcs=10):
    return poisson_case(shape, dirichlet, mcs)[1]


@functools.lru_cache(maxsize=None)
def _random_order():
    """75 k rows in random order: chunks whose rows touch more coarse columns than the workgroup has threads"""
    H = _poisson((45, 43, 39), "left", 10)
    return R.permute_hierarchy(H, R.level_perms(H, "random", seed=1))


@functools.lru_cache(maxsize=None)
def _lmax(H):
    from tests.cheby_ref import power_estimate
    return tuple(1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]) + (1.0,)


def _dev(H, env=(), sm_type="jacobi", **kw):
    """DeviceAMGMatrix created with `env` set in os.environ (restored afterwards: the switches are read by amgx_create)"""
    from ngsamg_amd.device import DeviceAMGMatrix
    sm = sm_type
    if sm.startswith("cheby"):
        kw.setdefault("cheb_lambda_max", list(_lmax(H)))
        kw.setdefault("cheb_degree", int(sm[5]) if sm[5:6].isdigit() else 2)
        if sm.endswith("f32"):
            kw["mat_prec"] = "single"
        sm = "cheby"
    env = dict(env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DeviceAMGMatrix(H, device=0, sm_type=sm, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _block(n, k=8, seed=0, H=None):
    """k random columns; with H: zero on the constrained dofs of its level 0, as a right-hand side of the cycle is"""
    B = np.random.default_rng(seed).standard_normal((k, n))
    return B if H is None else B * np.asarray(H.levels[0].free, dtype=np.float64)


def _down(dev, level, B, X=None, x_given=False, interleaved=False, device=False, fuse=False):
    """(X, BC) of DownMulti, both (k, n) whatever the layout and the kind of pointer handed to the library"""
    lay = (lambda M: np.array(M.T, order="C")) if interleaved else (lambda M: np.array(M, order="C"))
    Bin = lay(B)
    Xin = lay(X) if x_given else np.full_like(Bin, np.nan)
    if device:
        import torch
        Xd = torch.from_numpy(Xin).cuda()
        Xd, BCd = dev.DownMulti(level, torch.from_numpy(Bin).cuda(), Xd, x_given=x_given, interleaved=interleaved, fuse=fuse)
        torch.cuda.synchronize()
        Xo, BC = Xd.cpu().numpy(), BCd.cpu().numpy()
    else:
        Xo, BC = dev.DownMulti(level, Bin, Xin, x_given=x_given, interleaved=interleaved, fuse=fuse)
    return (np.ascontiguousarray(Xo.T), np.ascontiguousarray(BC.T)) if interleaved else (Xo, BC)


def _mult(dev, B, interleaved=False, device=False, graph=True, fuse=False):
    Bin = np.array(B.T if interleaved else B, order="C")
    if device:
        import torch
        Bd = torch.from_numpy(Bin).cuda()
        Xd = torch.full_like(Bd, float("nan"))
        dev.MultMulti(Bd, Xd, interleaved=interleaved, graph=graph, fuse=fuse)
        torch.cuda.synchronize()
        X = Xd.cpu().numpy()
    else:
        X = np.full_like(Bin, np.nan)
        dev.MultMulti(Bin, X, interleaved=interleaved, graph=graph, fuse=fuse)
    return np.ascontiguousarray(X.T) if interleaved else X


def _single(dev, B):
    X = np.empty_like(B)
    for j in range(B.shape[0]):
        dev.Mult(np.ascontiguousarray(B[j]), X[j])
    return X


def _base(fuse):
    """the keyword without the bit"""
    return {"down": True, "gs+down": "gs", "gs_block+down": "gs_block"}[fuse]


def _check_level(dev, level, fuse, lp_expect, form, mode, f32=False):
    lp = dev.level_paths(level)
    assert {k: lp[k] for k in lp_expect} == lp_expect, (level, lp)
    plan = dev.multi_level_plan(level, fuse)
    assert (plan["form"], plan["mode"], plan["float_image"], plan["note"]) == (form, mode, f32, ""), (level, plan)
    rows = 512 // (lp["lanes"] if mode != 1 else 1)
    ept = lp["ept"] if mode != 1 else None
    if ept:
        assert plan["lds_bytes"] == 8 * (rows * 4 + ept * 512), (plan, lp)
    assert 0 < plan["lds_bytes"] <= 40960, plan
    off = dev.multi_level_plan(level, _base(fuse))                  # without the bit: nothing
    assert off["out"] == [0] * 5 and off["note"] == "", off
    return lp, plan


# ---- 1. the stage, bit for bit ---------------------------------------------------------------------------------------------
def _sell(lanes, ept, **more):
    return dict({"kernel": "sell", "fused_block": 512, "lanes": lanes, "ept": ept}, **more)


def _cheb(lanes, ept=4):
    return {"kernel": "cheby-res", "fused_block": 512, "lanes": lanes, "ept": ept}


def _lanes(g):
    return (("AMGX_SELL_MAX_LANES", str(g)), ("AMGX_NO_LW", "1"))


COMPACT = ONE + NO_DENSE + (("AMGX_COMPACT_CHUNKS_MIN_ROWS", "1000"), ("AMGX_NO_LW", "1"))

# name: (hierarchy, sm_type, environment, fuse, {level: expected entries of level_paths}, (form, mode))
STAGE = {
    # MODE 0: one lane with EPT 6 and a partial last chunk (44 k rows = 85.7 chunks); folded and with the literal way up
    "jacobi-ept6": (lambda: _fd7((5, 2)), "jacobi", ONE, "down", {0: _sell(1, 6, folded=1)}, ("sell", 0)),
    "jacobi-ept6-nofold": (lambda: _fd7((5, 2)), "jacobi", ONE + (("AMGX_NO_FOLD", "1"),), "down", {0: _sell(1, 6, folded=0)}, ("sell", 0)),
    "jacobi-ept4-nohoist": (lambda: _fd7((2, 2)), "jacobi", ONE + (("AMGX_NO_EP_NT", "1"), ("AMGX_NO_EP_HOIST", "1")), "down", {0: _sell(1, 4)}, ("sell", 0)),
    "jacobi-ept4-nowdiag": (lambda: _fd7((2, 2)), "jacobi", ONE + (("AMGX_NO_WDIAG", "1"),), "down", {0: _sell(1, 4)}, ("sell", 0)),
    # (one lane per row: with the lanes its long rows would get, level 1 of this small problem has no fused down pass at all)
    "jacobi-kuhn": (lambda: _poisson((41, 37, 29)), "jacobi", ONE + NO_DENSE, "down", {0: _sell(1, 4), 1: {"kernel": "sell", "fused_block": 512, "lanes": 1}},
                    ("sell", 0)),
    "jacobi-g2": (_chain12, "jacobi", _lanes(2), "down", {0: _sell(2, 4)}, ("sell", 0)),
    "jacobi-g4": (_chain12, "jacobi", _lanes(4), "down", {0: _sell(4, 4)}, ("sell", 0)),
    "jacobi-g8": (_chain12, "jacobi", _lanes(8), "down", {0: _sell(8, 4)}, ("sell", 0)),
    "jacobi-slots": (_random_order, "jacobi", ONE, "down", {0: {"kernel": "sell", "fused_block": 512, "compact": 0}}, ("sell", 0)),
    "jacobi-compact": (lambda: _poisson((40, 38, 30), "right|top", 20), "jacobi", COMPACT, "down", {0: {"kernel": "sell", "fused_block": 512, "compact": 1}},
                       ("sell", 0)),
    "jacobi-rsum-sort": (lambda: _fd7((2, 2)), "jacobi", ONE + (("AMGX_RSUM_SORT", "1"),), "down", {0: _sell(1, 4)}, ("sell", 0)),
    # MODE 2: degree 1 and 2, one lane with EPT 4 / 6 and 2 / 4 / 8 lanes, fp64 and float image
    "cheby1-g1-ept4": (lambda: _fd7((2, 2)), "cheby1", ONE, "down", {0: _cheb(1)}, ("sell", 2)),
    "cheby2-g1-ept6": (lambda: _fd7((5, 2)), "cheby2", ONE, "down", {0: _cheb(1, 6)}, ("sell", 2)),
    "cheby2-g2": (_chain12, "cheby2", _lanes(2)[:1], "down", {0: _cheb(2)}, ("sell", 2)),
    "cheby1-g4": (_chain12, "cheby1", _lanes(4)[:1], "down", {0: _cheb(4)}, ("sell", 2)),
    "cheby2-g8": (_chain12, "cheby2", _lanes(8)[:1], "down", {0: _cheb(8)}, ("sell", 2)),
    "cheby2-g1-ept6-f32": (lambda: _fd7((5, 2)), "cheby2-f32", ONE, "down", {0: _cheb(1, 6)}, ("sell", 2)),
    "cheby1-g4-f32": (_chain12, "cheby1-f32", _lanes(4)[:1], "down", {0: _cheb(4)}, ("sell", 2)),
    "cheby2-g1-ept4-f32": (lambda: _fd7((2, 2)), "cheby2-f32", ONE, "down", {0: _cheb(1)}, ("sell", 2)),
    # MODE 1: the two forms of the block-hybrid down pass
    # (one lane per row: with the 8 lanes these small levels would get, the block-hybrid down pass has no fused residual + restriction)
    "hgs-21": (lambda: _poisson((21, 21, 21), "right|top", 20), "hgs", ONE + NO_DENSE, "gs+down", {0: {"gs_form": "hybrid"}}, (None, 1)),
    "hgs-33": (lambda: _poisson((33, 30, 28), "right|top", 20), "hgs", ONE + NO_DENSE + (("AMGX_NO_SELL_WINDOW", "1"),), "gs+down", {0: {"gs_form": "hybrid"}},
               (None, 1)),
    "hgs-sell": (lambda: _poisson((41, 37, 29)), "hgs", ONE + NO_DENSE + (("AMGX_NO_SELL_WINDOW", "1"),), "gs+down", {0: {"gs_form": "hybrid", "gs_down": "sell"}},
                 ("sell", 1)),
    "hgs-sell-win": (lambda: _poisson((41, 37, 29)), "hgs", ONE + NO_DENSE, "gs+down", {0: {"gs_form": "hybrid", "gs_down": "sell-win"}}, ("sell-win", 1)),
}


@pytest.mark.parametrize("name", list(STAGE))
def test_stage_bit_for_bit(name):
    problem, sm, env, fuse, levels, (form, mode) = STAGE[name]
    H = problem()
    dev = _dev(H, env, sm)
    for level, expect in levels.items():
        if sm == "hgs" and form is None:            # (the form the level happens to take; "hgs-sell" and "hgs-sell-win" fix one each)
            gd = dev.level_paths(level)["gs_down"]
            assert gd in ("sell", "sell-win"), (name, dev.level_paths(level))
            want = gd
        else:
            want = form
        lp, plan = _check_level(dev, level, fuse, expect, want, mode, f32=sm.endswith("f32"))
        if name == "jacobi-slots":
            assert lp["max_slots"] > lp["fused_block"], lp
        if sm.endswith("f32"):
            assert dev.matrix_info(level, "A32")["fmt"] == "sell" and plan["out"][3] == 1, plan
        n = dev.sizes[level]
        B = _block(n, 8, seed=level)
        Xr, BCr = _down(dev, level, B)                                    # without the bit: the single-vector functions per column
        assert np.isfinite(Xr).all() and np.isfinite(BCr).all() and BCr.any()
        modes = [False] if sm == "jacobi" else [False, True]
        worst = 0.0
        for given in modes:
            for k in (2, 4, 7, 8):
                for il in (False, True):
                    for on_dev in (False, True):
                        X, BC = _down(dev, level, B[:k], Xr[:k], x_given=given, interleaved=il, device=on_dev, fuse=fuse)
                        tag = (name, level, given, k, il, on_dev)
                        if sm.startswith("cheby") and not given:          # (the smooth itself is not bit-equal: 1e-13 per column)
                            ex = max(_rel(X[j], Xr[j]) for j in range(k))
                            ec = max(_rel(BC[j], BCr[j]) for j in range(k))
                            worst = max(worst, ex, ec)
                            assert ex <= 1e-13 and ec <= 1e-13, (tag, ex, ec)
                            continue
                        assert np.array_equal(X, Xr[:k]), tag
                        assert np.array_equal(BC, BCr[:k]), tag
            if sm.startswith("cheby") and not given:
                print(f"{name} level {level}: Chebyshev stage from zero, largest deviation per column {worst:.3e}")
            if given:                                                     # ... and without the bit the half stage is the same half
                X, BC = _down(dev, level, B[:3], Xr[:3], x_given=True)
                assert np.array_equal(BC, BCr[:3]) and np.array_equal(X, Xr[:3]), (name, level)
        if sm == "jacobi" and dev.is_folded(level):                       # amgx_cycle_down per column
            for j in (0, 5):
                x, bc = np.full(n, np.nan), np.full(dev.sizes[level + 1], np.nan)
                dev.CycleDown(level, np.ascontiguousarray(B[j]), x, bc)
                assert np.array_equal(x, Xr[j]) and np.array_equal(bc, BCr[j]), (name, level, j)
        if sm == "jacobi":                                                # x_given on a fused Jacobi level is refused
            from ngsamg_amd._lib import NgsAMGError
            with pytest.raises(NgsAMGError, match="forms x itself"):
                _down(dev, level, B[:2], Xr[:2], x_given=True, fuse=fuse)


# ---- 2. columns do not talk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jacobi-ept6", "cheby2-g2", "hgs-sell-win"])
def test_columns_do_not_talk(name):
    problem, sm, env, fuse, levels, (form, mode) = STAGE[name]
    dev = _dev(problem(), env, sm)
    level = 0
    _check_level(dev, level, fuse, levels[level], form, mode)
    n = dev.sizes[level]
    B = _block(n, 4, seed=7)
    X4, C4 = _down(dev, level, B, fuse=fuse)
    for j in range(4):
        for other in range(4):
            if other == j:
                continue
            X2, C2 = _down(dev, level, B[[j, other]], fuse=fuse)           # width 2, column first
            assert np.array_equal(X2[0], X4[j]) and np.array_equal(C2[0], C4[j]), (name, j, other)
        perm = [(j + s) % 4 for s in (1, 3, 0, 2)]                        # width 4, neighbours permuted
        Xp, Cp = _down(dev, level, B[perm], fuse=fuse)
        assert np.array_equal(Xp[2], X4[j]) and np.array_equal(Cp[2], C4[j]), (name, j)
    for bad in (0, 3):
        Bn = B.copy()
        Bn[bad] = np.nan
        Xn, Cn = _down(dev, level, Bn, fuse=fuse)
        assert np.isnan(Cn[bad]).all()
        keep = [j for j in range(4) if j != bad]
        assert np.array_equal(Xn[keep], X4[keep]) and np.array_equal(Cn[keep], C4[keep]), (name, bad)


# ---- 3. the cycle ------------------------------------------------------------------------------------------------------------
CYCLE = {
    # name: (hierarchy, sm_type, environment, fuse, bound against the oracle)
    "jacobi": (lambda: _fd7((5, 2)), "jacobi", ONE, "down", 1e-12),
    "jacobi-nofold": (lambda: _fd7((5, 2)), "jacobi", ONE + (("AMGX_NO_FOLD", "1"),), "down", 1e-12),
    "jacobi-kuhn": (lambda: _poisson((41, 37, 29)), "jacobi", ONE + NO_DENSE, "down", 1e-12),
    "cheby2": (lambda: _fd7((5, 2)), "cheby2", ONE, "down", 1e-12),
    "cheby1-g4": (_chain12, "cheby1", _lanes(4)[:1], "down", 1e-12),
    "hgs": (lambda: _poisson((21, 21, 21), "right|top", 20), "hgs", ONE + NO_DENSE, "gs+down", 1e-10),
    "hgs-sell-win": (lambda: _poisson((41, 37, 29)), "hgs", ONE + NO_DENSE, "gs+down", 1e-10),
}


def _oracle(H, dev, sm, B):
    from oracle.pyoracle import Oracle
    if sm == "hgs":
        from tests.hgs_oracle import hgs_levels
        lv, types = hgs_levels(H.levels, dev.hgs)
        orc = Oracle(lv, sm_type=types)
    elif sm.startswith("cheby"):
        from tests.cheby_ref import ChebyRef
        orc = ChebyRef(H, sm="cheby", degree=int(sm[5]), lambda_max=list(_lmax(H)))
    else:
        orc = Oracle(H.levels, sm_type="jacobi")
    return np.stack([orc.apply(np.array(b)) for b in B])


@pytest.mark.parametrize("name", list(CYCLE))
def test_cycle(name):
    problem, sm, env, fuse, tol = CYCLE[name]
    H = problem()
    dev = _dev(H, env, sm)
    base = _base(fuse)
    plans = [dev.multi_level_plan(l, fuse) for l in range(dev.n_levels - 1)]
    assert plans[0]["form"] != "literal" and plans[0]["note"] == "", plans
    for k in (2, 4, 7):
        p_on, p_off = dev.multi_plan(k, fuse), dev.multi_plan(k, base)
        assert p_on["fused"] == 1 and p_on["groups"] == p_off["groups"] and p_on["work_bytes"] > p_off["work_bytes"], (p_on, p_off)
    n = dev.sizes[0]
    B = _block(n, 7, seed=11, H=H)
    X = _mult(dev, B, fuse=fuse)
    ref = _oracle(H, dev, sm, B[:3])
    one = _single(dev, B)
    worst_o = max(_rel(X[j], ref[j]) for j in range(3))
    worst_s = max(_rel(X[j], one[j]) for j in range(7))
    print(f"{name}: cycle with the bit vs oracle {worst_o:.3e}, vs Mult {worst_s:.3e}")
    assert worst_o < tol and worst_s < 1e-12
    assert np.array_equal(X[6], one[6])                                  # the left-over column IS the single-vector path
    # graph replay = direct launches = a fresh handle, in both layouts and with device pointers
    assert np.array_equal(_mult(dev, B, fuse=fuse), X)
    assert np.array_equal(_mult(dev, B, graph=False, fuse=fuse), X)
    assert np.array_equal(_mult(dev, B, interleaved=True, device=True, fuse=fuse), X)
    assert np.array_equal(_mult(dev, B, interleaved=True, device=True, fuse=fuse), X)
    fresh = _dev(H, env, sm)
    assert np.array_equal(_mult(fresh, B, device=True, graph=False, fuse=fuse), X)
    assert np.array_equal(_mult(dev, B[:4], fuse=fuse), X[:4]) and np.array_equal(_mult(dev, B[:2], interleaved=True, fuse=fuse), X[:2])
    # a call without the bit afterwards is what a handle computes that never saw the bit
    never = _dev(H, env, sm)
    P0 = _mult(never, B, fuse=base)
    assert np.array_equal(_mult(dev, B, fuse=base), P0) and np.array_equal(_mult(dev, B, device=True, interleaved=True, fuse=base), P0)
    assert np.array_equal(_mult(dev, B, fuse=fuse), X)
    # k = 1 is Mult
    assert np.array_equal(_mult(dev, B[:1], fuse=fuse)[0], one[0])


# ---- 4. levels that stay literal --------------------------------------------------------------------------------------------
LITERAL = {
    # name: (hierarchy, sm_type, environment, fuse, level, expected entries of level_paths, note)
    "dia": (lambda: _fd7((2,), 64), "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), "down", 0, {"kernel": "dia"}, "diagonal image"),
    "fb1024": (lambda: _fd7((2,), 64), "jacobi", ONE + (("AMGX_FUSED_BLOCK", "1024"),), "down", 0, {"kernel": "sell", "fused_block": 1024}, "workgroup size"),
    "lw": (lambda: _poisson((41, 37, 29)), "jacobi", NO_DENSE + (("AMGX_LW_MIN_ROWS", "300"),), "down", 1, {"kernel": "sell-lw"}, "local-window image"),
    "mc": (lambda: _poisson((21, 21, 21), "right|top", 20), "gs", NO_DENSE, "gs+down", 0, {"gs_form": "mc"}, "multicolour sweep"),
}


@pytest.mark.parametrize("name", list(LITERAL))
def test_levels_that_stay_literal(name):
    problem, sm, env, fuse, level, expect, note = LITERAL[name]
    H = problem()
    dev = _dev(H, env, sm)
    lp = dev.level_paths(level)
    assert {k: lp[k] for k in expect} == expect, lp
    plan = dev.multi_level_plan(level, fuse)
    assert plan["form"] == "literal" and plan["out"] == [0] * 5 and plan["note"] == note, plan
    plans = [dev.multi_level_plan(l, fuse) for l in range(dev.n_levels - 1)]
    assert dev.multi_plan(4, fuse)["fused"] == 1
    n = dev.sizes[0]
    B = _block(n, 4, seed=5, H=H)
    with_bit, without = _mult(dev, B, fuse=fuse), _mult(dev, B, fuse=_base(fuse))
    if all(p["form"] == "literal" for p in plans):                        # nothing qualifies: the same launches
        assert np.array_equal(with_bit, without), name
        assert dev.multi_plan(4, fuse)["work_bytes"] == dev.multi_plan(4, _base(fuse))["work_bytes"]
    else:                                                                  # mixed per level: another level takes the fused pass
        print(f"{name}: mixed handle, with the bit vs without {_rel(with_bit, without):.3e}")
        assert _rel(with_bit, without) < 1e-12
    # the stage of the literal level is the column loop either way
    Bl = _block(dev.sizes[level], 4, seed=6)
    Xa, Ca = _down(dev, level, Bl, fuse=fuse)
    Xb, Cb = _down(dev, level, Bl)
    assert np.array_equal(Xa, Xb) and np.array_equal(Ca, Cb), name


# ---- 5. solvers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cheby2", "hgs"])
def test_solve_multi(name):
    from ngsamg_amd.krylov import NativeCGSolver
    problem, sm, env, fuse, _ = CYCLE[name]
    H = problem()
    dev = _dev(H, env, sm)
    assert dev.multi_level_plan(0, fuse)["form"] != "literal"
    B = _block(dev.sizes[0], 4, seed=2, H=H)
    its = {}
    for word in (fuse, _base(fuse)):
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
        X = np.zeros_like(B)
        cg.SolveMulti(B, X, fuse=word)
        its[word] = list(cg.iterations)
        assert np.isfinite(X).all()
    print(f"{name}: iterations with the bit {its[fuse]}, without {its[_base(fuse)]}")
    assert all(0 < a < 100 and abs(a - b) <= 1 for a, b in zip(its[fuse], its[_base(fuse)])), its


# ---- a leading dimension above the level size: k = 7 (groups 4 + 2 + 1) and k = 4, host arrays and device tensors -------------------
def test_stage_with_a_leading_dimension_above_n():
    from ngsamg_amd import _lib
    from tests.problems import padded_call
    problem, sm, env, fuse, levels, _ = STAGE["hgs-21"]
    dev = _dev(problem(), env, sm)
    lib, h, level = dev._lib, dev._h, 0
    assert dev.multi_level_plan(level, fuse)["form"] != "literal"
    n, nc = dev.sizes[level], dev.sizes[level + 1]
    B = _block(n, 7, seed=9)
    Xr, BCr = _down(dev, level, B)                       # the single-vector functions per column, ld = n
    bits = _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS | _lib.AMGX_MULTI_FUSE_DOWN
    for flag in (0, bits):
        for given in (False, True):
            for k in (7, 4):
                for device in (False, True):
                    def down(kk, a, flags):
                        rc = lib.amgx_down_multi(h, level, kk, a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1], int(given), flags | flag)
                        assert rc == 0, lib.amgx_last_error(h)
                    X0 = Xr[:k] if given else np.full((k, n), np.nan)
                    Bout, X, BC = padded_call(dev, down, [B[:k], X0, np.full((k, nc), np.nan)], device)
                    tag = (flag, given, k, device)
                    assert np.array_equal(Bout, B[:k]), tag
                    assert np.array_equal(X, Xr[:k]) and np.array_equal(BC, BCr[:k]), tag
