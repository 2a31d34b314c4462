"""AMGX_MULTI_FUSE_DOWN_F32 (fuse="gs+down_f32"): the multi-vector down pass on scalar Gauss-Seidel levels whose
images are single precision (mat_prec="single_gs_all", 5.21) -- sell, sell-win and the local-window form sell-lw of `rest`.

The problems and switches are those of tests/test_gpu_mat_prec_sgs.py (DOWN_FORMS): the (41, 37, 29) Kuhn Poisson problem under
"hgs" with AMGX_NO_DENSE_TAIL=1, whose `rest` takes each form of the fused residual + restriction; AMGX_LW_TEST_CAP=1000 leaves
some 256-row chunks of level 1 without a window (their slices carry 32-bit global columns; the longest list without the cap has 1803
columns); the (17, 17, 17) grid with AMGX_LW_MIN_ROWS=100 (level 0 sell-win, level 1 sell-lw in one cycle) and the (33, 33) grid (no
level with the fused residual + restriction: nothing changes).  Every case first asserts level_paths entry 33 ("gs_down") of its level.
References, all np.array_equal (per column the kernels keep the order of additions of the single-vector float kernels):
  * DownMulti under the word against DownMulti without a word (the column loop over the single-vector functions);
  * MultMulti under the word against Mult per column of the same handle, and against the AMGX_GS_F32_WIDE twin; the double handle
    differs (the float arrays really are read);
  * amgx_pcg_multi: per column the iteration count of amgx_pcg, true residual 1e-8 |b| at tol 1e-10.
No switch selects 4 lanes per row for the local-window image (the builder takes them only where 2 lanes do not fit the capacity),
none produces 4 entries of P per thread there or 6 on a sell / sell-win level of these sizes, and none makes a list longer than the
bound of width 4 (AMGX_LW_TEST_CAP only shortens lists): those shapes are covered by tests/test_multi_down_f32_cpu.py on the rule;
tools/bench_multi_rhs.py --down-f32 compares the 4-lane local-window form and the 6-entry sell-win form, which cfg 2 selects on levels 2
and 0, with the column loop bit for bit before it times them (profiles/r31/)."""
import functools
import os

import numpy as np
import pytest

from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
WIDE = {"AMGX_GS_F32_WIDE": "1"}
ONE = {"AMGX_SELL_MAX_LANES": "1"}
P3 = ((41, 37, 29), "right|top", 10)
G3 = ((17, 17, 17), "right|top", 20)
G2 = ((33, 33), "left|top", 5)
WORD, OLD = "gs+down_f32", "gs+down+f32"
NOTE = "single-precision Gauss-Seidel images"
CAP = 1000


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


# case -> (problem, environment, {level: form under the new word})
CASES = {
    "sell": (P3, _env(ONE, NO_DENSE, {"AMGX_NO_SELL_WINDOW": "1"}), {0: "sell"}),
    "sell-win": (P3, _env(ONE, NO_DENSE), {0: "sell-win"}),
    "sell-lw": (P3, _env(NO_DENSE, {"AMGX_LW_MIN_ROWS": "300"}), {1: "sell-lw"}),
    "sell-lw-cap": (P3, _env(NO_DENSE, {"AMGX_LW_MIN_ROWS": "300", "AMGX_LW_TEST_CAP": str(CAP)}), {1: "sell-lw"}),
    "3d": (G3, _env(NO_DENSE, {"AMGX_LW_MIN_ROWS": "100"}), {0: "sell-win", 1: "sell-lw"}),
}
NAMES = list(CASES)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, env=None, **kw):
    """DeviceAMGMatrix created with `env` set in os.environ (restored afterwards: the switches are read at create)"""
    from ngsamg_amd.device import DeviceAMGMatrix
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return DeviceAMGMatrix(H, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _problem(prob):
    """(problem, hierarchy, 7 right-hand sides of level 0)"""
    p, H = poisson_case(*prob)
    B = np.ascontiguousarray(np.stack([rhs(p, j) for j in range(7)]))
    B.setflags(write=False)
    return p, H, B


@functools.lru_cache(maxsize=None)
def _handle(name, prec="single"):
    """one handle per (case, "single" | "wide" | "double"), shared by the tests"""
    prob, env, _ = CASES[name]
    return _dev(_problem(prob)[1], _env(env, WIDE if prec == "wide" else {}), sm_type="hgs", mat_prec="double" if prec == "double" else "single_gs_all")


def _level_has_the_form(name, level, dev=None):
    """level_paths entry 33 first: the case cannot silently test another form"""
    dev = dev or _handle(name)
    form = CASES[name][2][level]
    lp = dev.level_paths(level)
    assert lp["gs_form"] == "hybrid" and lp["gs_down"] == form and lp["gs_split"] == 1, (name, level, lp)
    assert dev.cycle_info()["dense_level"] < 0, name
    return form


def _level_rhs(name, level, k=7):
    p, H, B = _problem(CASES[name][0])
    if level == 0:
        return np.array(B[:k])
    n = _handle(name).sizes[level]
    free = np.asarray(H.levels[level].free, dtype=np.float64)
    return np.ascontiguousarray(np.random.default_rng(100 + level).standard_normal((k, n)) * free)


def _down(dev, level, B, X=None, x_given=False, interleaved=False, device=False, fuse=False):
    """(X, BC) of DownMulti as (k, n) / (k, n_coarse) arrays whatever the layout and pointer kind handed to the library"""
    Bin = np.array(B.T if interleaved else B, order="C")
    Xin = None if X is None else np.array(X.T if interleaved else X, order="C")
    if device:
        import torch
        Bd = torch.from_numpy(Bin).cuda()
        Xd = None if Xin is None else torch.from_numpy(Xin).cuda()
        Xo, Co = dev.DownMulti(level, Bd, Xd, x_given=x_given, interleaved=interleaved, fuse=fuse)
        torch.cuda.synchronize()
        Xo, Co = Xo.cpu().numpy(), Co.cpu().numpy()
    else:
        Xo, Co = dev.DownMulti(level, Bin, Xin, x_given=x_given, interleaved=interleaved, fuse=fuse)
    return (np.ascontiguousarray(Xo.T), np.ascontiguousarray(Co.T)) if interleaved else (Xo, Co)


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


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_plan(name):
    single, wide, double = _handle(name), _handle(name, "wide"), _handle(name, "double")
    for level, form in CASES[name][2].items():
        _level_has_the_form(name, level)
        assert wide.level_paths(level) == single.level_paths(level), (name, level)
        assert single.gs_prec_info(level)["f32"] == 1 and wide.gs_prec_info(level)["wide"] == 1, (name, level)
        for dev, f32 in ((single, True), (wide, False)):
            plan = dev.multi_level_plan(level, fuse=WORD)
            assert plan["form"] == form and plan["mode"] == 1 and plan["float_image"] is f32 and plan["note"] == "" and not plan["folded_up"], (name, level, plan)
            assert plan["out"][0] == {"sell": 1, "sell-win": 2, "sell-lw": 5}[form], plan
            lanes, ept, W = plan["lanes"], plan["ept"], plan["lw_max_list"]
            if form == "sell-lw":                                # the LDS figure is the rule's at NV = 4
                assert lanes in (2, 4) and ept in (2, 4) and plan["lds_bytes"] == 8 * (W * 4 + (512 // lanes) * 4 + ept * 512) <= 163840, plan
            else:
                assert lanes == 1 and ept in (4, 6) and plan["lds_bytes"] == 8 * (512 * 4 + ept * 512), plan
            for old_word in (OLD, "gs_block+down+f32", "gs+down", "gs+down_dia"):
                old = dev.multi_level_plan(level, fuse=old_word)
                assert old["form"] == "literal" and old["out"] == [0] * 5 and old["note"] == NOTE, (name, level, old_word, old)
            assert dev.multi_level_plan(level, fuse="gs_block+down_f32")["form"] == form
            assert dev.multi_level_plan(level, fuse="gs+f32")["out"] == [0] * 5
        # the double handle: the new word changes nothing beyond what "gs+down+f32" and "gs+down" do
        new, base = double.multi_level_plan(level, fuse=WORD), double.multi_level_plan(level, fuse="gs+down")
        assert new == base == double.multi_level_plan(level, fuse=OLD), (name, level, new, base)
        assert new["note"] == ("local-window image" if form == "sell-lw" else ""), new
    # the work space counts the partial sums of the levels that now take the pass
    assert single.multi_plan(4, fuse=WORD)["work_bytes"] > single.multi_plan(4, fuse=OLD)["work_bytes"], name
    assert double.multi_plan(4, fuse=WORD) == double.multi_plan(4, fuse=OLD) == double.multi_plan(4, fuse="gs+down"), name
    for k in (2, 4, 5):
        plan = single.multi_plan(k, fuse=WORD)
        assert plan["fused"] == 1 and plan["note"] == "", plan


def test_the_cap_leaves_chunks_without_a_window():
    capped, full = _handle("sell-lw-cap").multi_level_plan(1, fuse=WORD), _handle("sell-lw").multi_level_plan(1, fuse=WORD)
    assert 0 < capped["lw_max_list"] <= CAP < full["lw_max_list"], (capped, full)


# ---- 2. DownMulti ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_down_multi(name):
    for level in CASES[name][2]:
        _level_has_the_form(name, level)
        B7 = _level_rhs(name, level)
        for prec in ("single", "wide"):
            dev = _handle(name, prec)
            Xl, Cl = _down(dev, level, B7)                       # the column loop: x after the sweep from zero, b_c
            assert np.isfinite(Xl).all() and np.isfinite(Cl).all() and np.linalg.norm(Cl) > 0, (name, level, prec)
            Xg, Cg = _down(dev, level, B7, Xl, x_given=True)
            assert np.array_equal(Cg, Cl), (name, level, prec, "the column loop with x given")
            for k in (2, 4, 5, 7):
                for interleaved in (False, True):
                    for device in (False, True):
                        Xf, Cf = _down(dev, level, B7[:k], interleaved=interleaved, device=device, fuse=WORD)
                        assert np.array_equal(Xf, Xl[:k]) and np.array_equal(Cf, Cl[:k]), (name, level, prec, k, interleaved, device, _rel(Cf, Cl[:k]))
                        Xf, Cf = _down(dev, level, B7[:k], Xl[:k], x_given=True, interleaved=interleaved, device=device, fuse=WORD)
                        assert np.array_equal(Xf, Xl[:k]) and np.array_equal(Cf, Cl[:k]), (name, level, prec, k, interleaved, device, "x given", _rel(Cf, Cl[:k]))
        assert np.array_equal(_down(_handle(name, "wide"), level, B7)[1], _down(_handle(name), level, B7)[1]), (name, level, "twin")
        assert not np.array_equal(_down(_handle(name, "double"), level, B7)[1], _down(_handle(name), level, B7)[1]), (name, level, "double")


# ---- 3. MultMulti ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mult_multi(name):
    for level in CASES[name][2]:
        _level_has_the_form(name, level)
    single, wide, double = _handle(name), _handle(name, "wide"), _handle(name, "double")
    B = _level_rhs(name, 0, 5)
    one = _single(single, B)
    assert np.isfinite(one).all() and np.linalg.norm(one) > 0
    for k in (2, 4, 5):
        for interleaved, device, graph in ((False, False, True), (False, False, True), (True, True, True), (False, True, False), (True, False, False)):
            X = _mult(single, B[:k], interleaved, device, graph, WORD)      # (the second run replays the captured graph)
            assert np.array_equal(X, one[:k]), (name, k, interleaved, device, graph, max(_rel(X[j], one[j]) for j in range(k)))
    Xw = _mult(wide, B, fuse=WORD)
    assert np.array_equal(Xw, one), (name, "twin", max(_rel(Xw[j], one[j]) for j in range(5)))
    assert np.array_equal(_mult(single, B, fuse=OLD), one) and np.array_equal(_mult(single, B, fuse="gs+f32"), one), name
    Xd = _mult(double, B, fuse=WORD)
    assert np.array_equal(Xd, _mult(double, B, fuse="gs+down")), (name, "double handle")
    assert min(_rel(one[j], Xd[j]) for j in range(5)) >= 1e-10, name


def test_a_handle_without_the_fused_residual_keeps_its_plan():
    """(33, 33): no level runs the fused residual + restriction, the word changes nothing and the columns still equal Mult"""
    p, H, B7 = _problem(G2)
    dev = _dev(H, NO_DENSE, sm_type="hgs", mat_prec="single_gs_all")
    assert dev.gs_prec_info(0)["f32"] == 1
    for level in range(dev.n_levels - 1):
        assert dev.level_paths(level)["gs_down"] is None
        plan = dev.multi_level_plan(level, fuse=WORD)
        assert plan["form"] == "literal" and plan["note"] == NOTE and plan == dev.multi_level_plan(level, fuse=OLD), (level, plan)
    assert dev.multi_plan(4, fuse=WORD) == dev.multi_plan(4, fuse=OLD)
    B = np.array(B7[:5])
    assert np.array_equal(_mult(dev, B, fuse=WORD), _single(dev, B))


# ---- 4. amgx_pcg_multi ----------------------------------------------------------------------------------------------------------------
def test_solve_multi():
    from ngsamg_amd.krylov import NativeCGSolver
    name = "3d"
    for level in CASES[name][2]:
        _level_has_the_form(name, level)
    p, H, B7 = _problem(G3)
    dev = _handle(name)
    free = np.asarray(p.free, dtype=np.float64)
    n = dev.sizes[0]
    rng = np.random.default_rng(0)
    B = np.ascontiguousarray(np.stack([B7[0], rng.standard_normal(n) * free, rng.standard_normal(n) * free, np.zeros(n)]))
    tol = 1e-10
    cg = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
    X = np.zeros_like(B)
    cg.SolveMulti(B, X, fuse=WORD)
    its, errs = cg.iterations, cg.errors
    assert its[3] == 0 and not X[3].any()
    A = H.levels[0].A.to_scipy()
    f = free.astype(bool)
    for j in range(3):
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        print(f"column {j}: iterations multi {its[j]} single {one.iterations}")
        assert its[j] == one.iterations, (j, its[j], one.iterations)
        assert errs[j][-1] <= tol * errs[j][0], j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j
