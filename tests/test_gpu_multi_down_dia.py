"""AMGX_MULTI_FUSE_DOWN_DIA (fuse="down_dia"): the fused multi-vector down pass on levels with the symmetric diagonal
image, 512-row chunks (dia_pre_restrict_nv_kernel) and box chunks (dia_box_pre_restrict_nv_kernel), and the folded way up on them.

Every test first asserts through level_paths and multi_level_plan that the level takes the kernel it means to test, and that under
fuse="down" the same level is still "literal" with the note "diagonal image".

1. The stage (DownMulti) with the word against the stage without any bit (the column loop over the single-vector kernel),
   array_equal per column for X and BC: per column the kernels form the same expressions in the same order, the partial sums are
   grouped by the same chunks and added in the same order.  No tolerance.
2. The box stage against the row-chunk stage of the same hierarchy: X equal bit for bit, BC within 1e-13 relative (the partial sums
   are grouped by box instead of by 512 rows: the bound of tests/test_gpu_dia_box.py).
3. No column sees its neighbours: other widths, permuted neighbours, a NaN column.
4. The cycle (MultMulti) against the oracle and against Mult per column (1e-12), graph replay = direct launches = a
   fresh handle, later calls with "down" or without a bit = a handle that never saw the word, k = 1 = Mult, the work space; a level
   0 with a local-window image of Q folds the way up under the new word only.
5. PCG: iteration counts with the word and with fuse=True differ by one at most.
"""
import functools

import numpy as np
import pytest

from tests.test_gpu_multi_down import NO_DENSE, ONE, _block, _dev, _down, _fd7, _hand, _mult, _poisson, _rel, _single

pytestmark = pytest.mark.gpu

WORD = "down_dia"
ROW = (("AMGX_DIA_MIN_ROWS", "0"),)
BOX = (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_DIA_BOX_MIN_ROWS", "0"), ("AMGX_DIA_MAX_FILL", "1.5"))        # tests/test_gpu_dia_box.py
NO_BOX = BOX + (("AMGX_NO_DIA_BOX", "1"),)
VARIANTS = {"folded": (), "nofold": (("AMGX_NO_FOLD", "1"),), "plain-ep": (("AMGX_NO_EP_NT", "1"), ("AMGX_NO_EP_HOIST", "1"))}


def _fd9():
    return _hand("fd9", (130, 110), (2, 2))


def _wide():
    """7-point stencil on lines of 60 rows, 5 entries of P per row: 2400 entries in a box of 8 lines, more than the 4 * 512 one
    pass of the box kernel's restriction takes (the 41-row lines of _fd7((5, 2)) give 1640)"""
    return _hand("fd7", (60, 20, 12), (5, 2))


def _row(**more):
    return dict({"kernel": "dia", "fused_block": 512, "lanes": 1}, **more)


def _boxed(**more):
    return dict({"kernel": "dia", "fused_block": 512, "compact": 2}, **more)


# name: (hierarchy, environment, expected entries of level_paths of level 0, form, rows of a full box where the grid is known)
STAGE = {
    "row-ept4": (lambda: _fd7((2, 2)), ROW, _row(dia_k=3, ept=4, compact=0), "dia", None),
    "row-ept6": (lambda: _fd7((5, 2)), ROW, _row(dia_k=3, ept=6, compact=0), "dia", None),
    "row-kuhn": (lambda: _poisson((41, 37, 29)), ROW, _row(dia_k=7, compact=0), "dia", None),
    "row-fd9": (_fd9, BOX, _row(dia_k=4, compact=0), "dia", None),                  # a diagonal image the boxes refuse
    "row-compact": (lambda: _fd7((5, 2)), ROW + (("AMGX_COMPACT_CHUNKS_MIN_ROWS", "0"),), _row(dia_k=3, ept=6, compact=1), "dia", None),
    "box-6x5x70": (lambda: _poisson((6, 5, 70), "right|top", 10), BOX, _boxed(dia_k=7), "dia-box", None),
    "box-9x9x9": (lambda: _poisson((9, 9, 9), "right|top", 10), BOX, _boxed(dia_k=7), "dia-box", None),
    "box-7x130": (lambda: _poisson((7, 130), "left|top", 5), BOX, _boxed(dia_k=3), "dia-box", None),
    "box-ept6": (lambda: _fd7((5, 2)), BOX, _boxed(dia_k=3), "dia-box", 41 * 8),
    "box-wide": (_wide, BOX, _boxed(dia_k=3), "dia-box", 60 * 8),
    "box-2x2": (lambda: _poisson((6, 5, 70), "right|top", 10), BOX + (("AMGX_DIA_BOX_SHAPE", "2x2"),), _boxed(dia_k=7), "dia-box", None),
}


def _check_level(dev, level, expect, form, box_rows=None):
    lp = dev.level_paths(level)
    assert {k: lp[k] for k in expect} == expect, (level, lp)
    plan = dev.multi_level_plan(level, WORD)
    assert (plan["form"], plan["mode"], plan["float_image"], plan["note"]) == (form, 0, False, ""), (level, plan)
    assert plan["out"][0] == (3 if form == "dia" else 4), plan
    if form == "dia":
        assert plan["lds_bytes"] == 8 * (512 * 4 + lp["ept"] * 512) <= 40960, (plan, lp)
    else:
        if box_rows:
            assert plan["lds_bytes"] == 8 * (box_rows * 4 + max(box_rows * 4, lp["max_entries"])), (plan, lp)
        # (a full box holds at least the average box; r and x_j of 4 columns; 160 KiB at most)
        assert 8 * 2 * 4 * -(-dev.sizes[level] // lp["chunks"]) <= plan["lds_bytes"] <= 163840, (plan, lp)
    old = dev.multi_level_plan(level, "down")                        # AMGX_MULTI_FUSE_DOWN alone: as before
    assert old["form"] == "literal" and old["out"] == [0] * 5 and old["note"] == "diagonal image", old
    off = dev.multi_level_plan(level, True)                          # without any down bit: nothing
    assert off["out"] == [0] * 5 and off["note"] == "", off
    return lp, plan


# ---- 1. the stage, bit for bit ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stage_ref(name, variant):
    """(B, X, BC) of the column loop over the single-vector kernel, computed once per (case, variant) and left unchanged"""
    problem, env, expect, form, box_rows = STAGE[name]
    dev = _dev(problem(), env + VARIANTS[variant])
    B = _block(dev.sizes[0], 8, seed=1)
    X, BC = _down(dev, 0, B)
    for a in (B, X, BC):
        a.setflags(write=False)
    return B, X, BC


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(STAGE))
def test_stage_bit_for_bit(name, variant):
    problem, env, expect, form, box_rows = STAGE[name]
    dev = _dev(problem(), env + VARIANTS[variant])
    lp, plan = _check_level(dev, 0, expect, form, box_rows)
    assert dev.is_folded(0) == (variant != "nofold")
    if name == "box-wide":
        assert lp["max_entries"] > 4 * 512, lp                        # the entry loop of the restriction runs more than once
    if name == "box-ept6":
        assert lp["max_entries"] > 3 * 41 * 8, lp
    B, Xr, BCr = _stage_ref(name, variant)
    assert np.isfinite(Xr).all() and np.isfinite(BCr).all() and BCr.any()
    for k in (2, 4, 7, 8):
        for il in (False, True):
            for on_dev in (False, True):
                X, BC = _down(dev, 0, B[:k], interleaved=il, device=on_dev, fuse=WORD)
                tag = (name, variant, k, il, on_dev)
                for j in range(k):
                    assert np.array_equal(X[j], Xr[j]), tag + (j, "X")
                    assert np.array_equal(BC[j], BCr[j]), tag + (j, "BC")
    # under "down" alone the stage is the column loop
    X, BC = _down(dev, 0, B[:4], fuse="down")
    assert np.array_equal(X, Xr[:4]) and np.array_equal(BC, BCr[:4]), (name, variant)
    from ngsamg_amd._lib import NgsAMGError                           # x_given on a fused Jacobi level is refused, as under "down"
    with pytest.raises(NgsAMGError, match="forms x itself"):
        _down(dev, 0, B[:2], Xr[:2], x_given=True, fuse=WORD)


# ---- 2. box chunks against row chunks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box-6x5x70", "box-9x9x9", "box-7x130", "box-ept6", "box-wide", "box-2x2"])
def test_box_stage_against_row_chunk_stage(name):
    problem, env, expect, form, box_rows = STAGE[name]
    H = problem()
    box = _dev(H, env)
    old = _dev(H, NO_BOX)
    _check_level(box, 0, expect, "dia-box", box_rows)
    _check_level(old, 0, _row(dia_k=expect["dia_k"], compact=0), "dia")
    B = _block(box.sizes[0], 4, seed=2)
    for k in (2, 4):
        Xb, Cb = _down(box, 0, B[:k], fuse=WORD)
        Xo, Co = _down(old, 0, B[:k], fuse=WORD)
        assert np.array_equal(Xb, Xo), (name, k)
        worst = max(_rel(Cb[j], Co[j]) for j in range(k))
        print(f"{name}: k = {k}: box vs row chunks, b_c {worst:.3e}")
        assert worst < 1e-13, (name, k, worst)


# ---- 3. columns do not talk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["row-kuhn", "box-6x5x70"])
def test_columns_do_not_talk(name):
    problem, env, expect, form, box_rows = STAGE[name]
    dev = _dev(problem(), env)
    _check_level(dev, 0, expect, form, box_rows)
    B = _block(dev.sizes[0], 7, seed=7)
    X7, C7 = _down(dev, 0, B, fuse=WORD)                                 # groups 4 + 2 + a single column
    X4, C4 = _down(dev, 0, B[:4], fuse=WORD)
    assert np.array_equal(X7[:4], X4) and np.array_equal(C7[:4], C4), name
    for j in range(4):
        for other in range(4):
            if other == j:
                continue
            X2, C2 = _down(dev, 0, B[[j, other]], fuse=WORD)              # width 2, column first
            assert np.array_equal(X2[0], X4[j]) and np.array_equal(C2[0], C4[j]), (name, j, other)
        perm = [(j + s) % 4 for s in (1, 3, 0, 2)]                        # width 4, neighbours permuted
        Xp, Cp = _down(dev, 0, B[perm], fuse=WORD)
        assert np.array_equal(Xp[2], X4[j]) and np.array_equal(Cp[2], C4[j]), (name, j)
    for j in (4, 5, 6):                                                   # the same column in a group of 2 and alone (k = 7), and in a group of 4
        Xq, Cq = _down(dev, 0, B[[0, 1, j, 2]], fuse=WORD)
        assert np.array_equal(Xq[2], X7[j]) and np.array_equal(Cq[2], C7[j]), (name, j)
    for bad in (0, 3):
        Bn = B[:4].copy()
        Bn[bad] = np.nan
        Xn, Cn = _down(dev, 0, Bn, fuse=WORD)
        assert np.isnan(Cn[bad]).all()
        keep = [j for j in range(4) if j != bad]
        assert np.array_equal(Xn[keep], X4[keep]) and np.array_equal(Cn[keep], C4[keep]), (name, bad)


# ---- 4. the cycle ------------------------------------------------------------------------------------------------------------
LW = (("AMGX_LW_MIN_ROWS", "300"),)
# name: (hierarchy, environment, {level: (form, note) under the word}, folded_up of level 0 under the word / under "down")
CYCLE = {
    "row": (lambda: _fd7((5, 2)), ROW, {0: ("dia", "")}, (True, False)),
    "box": (lambda: _poisson((6, 5, 70), "right|top", 10), BOX, {0: ("dia-box", "")}, (True, False)),
    # a mixed handle: level 0 fused (it has a local-window image of Q beside the plain one), level 1 literal
    "kuhn-mixed": (lambda: _poisson((41, 37, 29)), ROW + LW + NO_DENSE, {0: ("dia", ""), 1: ("literal", "local-window image")}, (True, False)),
    # no diagonal image: level 0 takes the sell form under both words; its Q has the local-window image, so only the new word folds
    "sell-qlw": (lambda: _poisson((41, 37, 29)), LW + NO_DENSE, {0: ("sell", ""), 1: ("literal", "local-window image")}, (True, False)),
}


@pytest.mark.parametrize("name", list(CYCLE))
def test_cycle(name):
    from oracle.pyoracle import Oracle
    problem, env, levels, (fold_new, fold_old) = CYCLE[name]
    H = problem()
    dev = _dev(H, env)
    for level, (form, note) in levels.items():
        plan = dev.multi_level_plan(level, WORD)
        assert (plan["form"], plan["note"]) == (form, note), (level, plan)
        old = dev.multi_level_plan(level, "down")
        if form in ("dia", "dia-box"):
            assert dev.level_paths(level)["kernel"] == "dia"
            assert old["form"] == "literal" and old["note"] == "diagonal image" and old["out"] == [0] * 5, old
        elif form == "literal":
            assert dev.level_paths(level)["kernel"] == "sell-lw" and old["form"] == "literal" and old["note"] == note, old
        else:
            assert old["form"] == form, old
    if name in ("kuhn-mixed", "sell-qlw"):
        assert dev.matrix_info(0, "QLW")["fmt"] == "sell-lw", "level 0 did not take the local-window image of Q"
    assert dev.is_folded(0)
    assert dev.multi_level_plan(0, WORD)["folded_up"] is fold_new and dev.multi_level_plan(0, "down")["folded_up"] is fold_old
    for k in (2, 4, 7):
        p_new, p_old, p_off = dev.multi_plan(k, WORD), dev.multi_plan(k, "down"), dev.multi_plan(k, True)
        assert p_new["fused"] == 1 and p_new["groups"] == p_old["groups"] == p_off["groups"], (p_new, p_old, p_off)
        if levels[0][0] == "sell":                                      # (the same partial sums under both words: only the way up differs)
            assert p_new["work_bytes"] == p_old["work_bytes"] > p_off["work_bytes"], (p_new, p_old, p_off)
        else:
            assert p_new["work_bytes"] > p_old["work_bytes"] >= p_off["work_bytes"], (p_new, p_old, p_off)
    n = dev.sizes[0]
    B = _block(n, 7, seed=11, H=H)
    X = _mult(dev, B, fuse=WORD)
    orc = Oracle(H.levels, sm_type="jacobi")
    ref = np.stack([orc.apply(np.array(b)) for b in B[:3]])
    one = _single(dev, B)
    worst_o = max(_rel(X[j], ref[j]) for j in range(3))
    worst_s = max(_rel(X[j], one[j]) for j in range(7))
    print(f"{name}: cycle with the word vs oracle {worst_o:.3e}, vs Mult {worst_s:.3e}")
    assert worst_o < 1e-12 and worst_s < 1e-12
    assert np.array_equal(X[6], one[6])                                  # the left-over column IS the single-vector path
    # graph replay = direct launches = a fresh handle, in both layouts and with device pointers
    assert np.array_equal(_mult(dev, B, fuse=WORD), X)
    assert np.array_equal(_mult(dev, B, graph=False, fuse=WORD), X)
    assert np.array_equal(_mult(dev, B, interleaved=True, device=True, fuse=WORD), X)
    assert np.array_equal(_mult(dev, B, interleaved=True, device=True, fuse=WORD), X)
    fresh = _dev(H, env)
    assert np.array_equal(_mult(fresh, B, device=True, graph=False, fuse=WORD), X)
    assert np.array_equal(_mult(dev, B[:4], fuse=WORD), X[:4]) and np.array_equal(_mult(dev, B[:2], interleaved=True, fuse=WORD), X[:2])
    # later calls with "down" or without any bit are what a handle computes that never saw the new word
    never = _dev(H, env)
    for word in ("down", True):
        P0 = _mult(never, B, fuse=word)
        assert np.array_equal(_mult(dev, B, fuse=word), P0), (name, word)
        assert np.array_equal(_mult(dev, B, device=True, interleaved=True, fuse=word), P0), (name, word)
        assert np.array_equal(_mult(dev, B, fuse=WORD), X), (name, word)
    # k = 1 is Mult
    assert np.array_equal(_mult(dev, B[:1], fuse=WORD)[0], one[0])


# ---- 5. solvers ---------------------------------------------------------------------------------------------------------------
def test_solve_multi():
    from ngsamg_amd.krylov import NativeCGSolver
    H = _poisson((6, 5, 70), "right|top", 10)
    dev = _dev(H, BOX)
    _check_level(dev, 0, _boxed(dia_k=7), "dia-box")
    B = _block(dev.sizes[0], 4, seed=2, H=H)
    its = {}
    for word in (WORD, True):
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
        X = np.zeros_like(B)
        cg.SolveMulti(B, X, fuse=word)
        its[word] = list(cg.iterations)
        assert np.isfinite(X).all()
    print(f"box: iterations with the word {its[WORD]}, with fuse=True {its[True]}")
    assert all(0 < a < 100 and abs(a - b) <= 1 for a, b in zip(its[WORD], its[True])), its
