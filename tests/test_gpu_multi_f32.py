"""AMGX_MULTI_FUSE_F32 (fuse="gs+f32" / "gs_block+f32"): fused multi-vector cycles on Gauss-Seidel levels whose sweeps
read single-precision images -- scalar levels with mat_prec="single_gs_all" (5.21), 2x2 / 3x3 / 6x6 levels with mat_prec="single_gs" (5.17).

The problems are those of tests/test_gpu_mat_prec_sgs.py and tests/test_gpu_mat_prec_gs.py.  Every case first asserts, through
level_paths / gs_prec_info / level_extra, that level 0 has the form its name says and reads float images.  References:
  * the single-vector step of the SAME handle: a column of SmoothMulti equals Smooth, a column of MultMulti equals Mult, bit for bit;
  * the AMGX_GS_F32_WIDE twin (the fp64 multi-vector kernels on the rounded values), bit for bit; the double handle differs by at
    least 1e-10 relative (the float images really are read);
  * PCG: per column the iteration count of amgx_pcg on that handle, the error history within rtol 1e-6 (the tolerance of
    tests/test_gpu_multi_gs.py for the double handle), true residual 1e-8 |b| at tol 1e-10 (as there).
The scalar multicolour form has no switch against the split images; its no-split cases are the hierarchies with an l1 inverse
diagonal of tests/test_gpu_mat_prec_sgs.py ("mc7", "mc31"), where the level never gets them."""
import functools
import os

import numpy as np
import pytest

from tests import reorder as R
from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
WIDE = {"AMGX_GS_F32_WIDE": "1"}
NOTE = "single-precision Gauss-Seidel images (level 0)"
LANE_LENGTHS = {1: 17, 2: 32, 4: 64, 8: 128, 16: 256}                    # one longest row per G (tests/test_gpu_gs_paths.py)
GRIDS = {"3d": ((17, 17, 17), "right|top", 20), "2d": ((33, 33), "left|top", 5), "3d-odd": ((24, 22, 20), "right|top", 20)}
BLOCK_SHAPES = {"3d": ((14, 13, 12), False, 3), "rot": ((12, 11, 10), True, 6), "2d": ((40, 36), False, 2)}
BC = {"AMGX_BGSB_BC_MIN_ROWS": "0"}
BSELL = {"AMGX_BGS_BSELL_MIN": "1"}


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


# block form -> (smoother, environment, gs_form of level 0, gs_split of level 0): tests/test_gpu_mat_prec_gs.py
BLOCK_FORMS = {
    "hybrid": ("hgs", NO_DENSE, "hybrid-block", 1),
    "hybrid-nosplit": ("hgs", _env(NO_DENSE, {"AMGX_BGSB_NO_SPLIT": "1"}), "hybrid-block", 0),
    "hybrid-compact": ("hgs", _env(NO_DENSE, {"AMGX_BGSB_COMPACT": "1"}), "hybrid-block", 1),
    "bc": ("hgs", _env(NO_DENSE, BC), "block-coloured", 1),
    "bc-nosplit": ("hgs", _env(NO_DENSE, BC, {"AMGX_BGSB_NO_SPLIT": "1"}), "block-coloured", 0),
    "mc": ("gs", _env(NO_DENSE, BSELL), "mc-block-bsell", 1),
    "mc-nosplit": ("gs", _env(NO_DENSE, BSELL, {"AMGX_NO_BGS_SPLIT": "1"}), "mc-block-bsell", 0),
}

# case name -> (kind, problem key, smoother, environment, gs_form of level 0, gs_split of level 0)
CASES = {}
for _g in GRIDS:
    CASES[f"{_g}-hgs"] = ("scalar", _g, "hgs", NO_DENSE, "hybrid", 1)
    CASES[f"{_g}-hgs-nosplit"] = ("scalar", _g, "hgs", _env(NO_DENSE, {"AMGX_GSB_NO_SPLIT": "1"}), "hybrid", 0)
    CASES[f"{_g}-gs"] = ("scalar", _g, "gs", NO_DENSE, "mc", 1)
for _l in (7, 31):
    CASES[f"mc{_l}-gs-nosplit"] = ("scalar", _l, "gs", NO_DENSE, "mc", 0)
for _s in BLOCK_SHAPES:
    for _f, (_sm, _e, _form, _split) in BLOCK_FORMS.items():
        CASES[f"b{_s}-{_f}"] = ("block", _s, _sm, _e, _form, _split)
SCALAR = [n for n, c in CASES.items() if c[0] == "scalar"]
BLOCK = [n for n, c in CASES.items() if c[0] == "block"]
ALL = SCALAR + BLOCK


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
def _problem(name):
    """(hierarchy, free mask of the scalar dofs of level 0, 5 right-hand sides)"""
    kind, key = CASES[name][:2]
    if kind == "block":
        grid, rot, bs = BLOCK_SHAPES[key]
        p, H = elasticity_case(grid, rot, 10)
        assert H.levels[0].A.br == bs
        free = np.repeat(p.free, p.bs).astype(np.float64)
        B = np.stack([rhs(p, j) for j in range(5)])
    elif isinstance(key, int):                               # multicolour with an l1 inverse diagonal: no split
        A = R.gs_scalar_case(key, "identity")[0]
        H = R.gs_hierarchy(A, np.ones(A.shape[0], np.uint8), l1_dinv=True, seed=key)
        free = np.ones(A.shape[0])
        B = np.random.default_rng(key).standard_normal((5, A.shape[0]))
    else:
        p, H = poisson_case(*GRIDS[key])
        free = np.asarray(p.free, dtype=np.float64)
        B = np.stack([rhs(p, j) for j in range(5)])
    B = np.ascontiguousarray(B)
    B.setflags(write=False)
    return H, free, B


def _words(name):
    """(mat_prec, the word with the new bit, the word without it)"""
    return ("single_gs", "gs_block+f32", "gs_block") if CASES[name][0] == "block" else ("single_gs_all", "gs+f32", "gs")


@functools.lru_cache(maxsize=None)
def _handle(name, prec="single"):
    """one handle per (case, "single" | "wide" | "double"), shared by the tests"""
    sm, env = CASES[name][2:4]
    env = _env(env, WIDE if prec == "wide" else {})
    return _dev(_problem(name)[0], env, sm_type=sm, mat_prec="double" if prec == "double" else _words(name)[0])


def _float_level0(name, dev=None):
    """level 0 of the case has the form its name says and its sweeps read float images"""
    dev = dev or _handle(name)
    kind, _, sm, env, form, split = CASES[name]
    lp, ex = dev.level_paths(0), dev.level_extra(0)
    assert lp["gs_form"] == form and lp["gs_split"] == split, (name, lp)
    assert ex["gs_f32"] == 1 and ex["gs_f32_images"] >= 2 and ex["gs_f32_bytes"] > 0, (name, ex)
    assert dev.cycle_info()["dense_level"] < 0, name
    if kind == "scalar":
        info = dev.gs_prec_info(0)
        assert info["f32"] == 1 and info["wide"] == 0 and info["bytes"] > 0, (name, info)
        want = ({"full"} if form == "hybrid" else {"sell"}) | (({"lowin", "rest"} if form == "hybrid" else {"lower", "upper"}) if split else {"A"})
        assert want <= set(info["images"]), (name, info)
    else:
        assert dev.matrix_info(0, "A32")["fmt"] == "bsell", name
    return lp


def _mult(dev, B, interleaved=False, device=False, graph=True, fuse=False):
    """X = C B through MultMulti; B and the result are (k, n) whatever the layout handed to the library"""
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


def _smooth_multi(dev, level, X0, B, x_zero, back, interleaved, device, fuse):
    Xin = np.array(X0.T if interleaved else X0, order="C")
    Bin = np.array(B.T if interleaved else B, order="C")
    if device:
        import torch
        Xd, Bd = torch.from_numpy(Xin).cuda(), torch.from_numpy(Bin).cuda()
        dev.SmoothMulti(level, Xd, Bd, x_zero=x_zero, back=back, interleaved=interleaved, fuse=fuse)
        torch.cuda.synchronize()
        Xin = Xd.cpu().numpy()
    else:
        dev.SmoothMulti(level, Xin, Bin, x_zero=x_zero, back=back, interleaved=interleaved, fuse=fuse)
    return np.ascontiguousarray(Xin.T) if interleaved else Xin


def _check_plan(dev, word, old_word, note=NOTE):
    """fused under the new word (groups 4 / 2 / 1, empty note); under the old word the column loop with the old note"""
    for k, groups in ((1, [1]), (2, [2]), (4, [4]), (5, [4, 1])):
        plan = dev.multi_plan(k, fuse=word)
        assert plan["fused"] == 1 and plan["groups"] == groups and plan["note"] == "", (k, word, plan)
        old = dev.multi_plan(k, fuse=old_word)
        assert old["fused"] == 0 and old["groups"] == [1] * k and note in old["note"], (k, old_word, old)


def _check_sweeps(dev, free, word, seed, level=0, twin=None):
    """a column of SmoothMulti under `word` is Smooth of the same handle, bit for bit: forward / backward, x_zero on / off,
    interleaved / column-major, host arrays and device tensors; `twin`: its SmoothMulti gives the same bits"""
    n = dev.sizes[level]
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((5, n)) * free
    Xs = rng.standard_normal((5, n)) * free
    for back in (False, True):
        for x_zero in (False, True):
            X0 = np.zeros_like(Xs) if x_zero else Xs
            one = X0.copy()
            for j in range(5):
                dev.Smooth(level, one[j], np.ascontiguousarray(B[j]), np.zeros(n), x_zero=x_zero, back=back)
            assert not np.array_equal(one, X0)
            for k, interleaved, device in ((2, False, False), (4, True, False), (5, False, True), (4, True, True), (5, True, False)):
                X = _smooth_multi(dev, level, X0[:k], B[:k], x_zero, back, interleaved, device, word)
                assert np.array_equal(X, one[:k]), (back, x_zero, k, interleaved, device, float(np.abs(X - one[:k]).max()))
            if twin is not None:
                assert np.array_equal(_smooth_multi(twin, level, X0[:4], B[:4], x_zero, back, True, True, word), one[:4]), (back, x_zero, "twin")


# ---- 1. the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_plan(name):
    mat_prec, word, old_word = _words(name)
    for prec in ("single", "wide"):
        dev = _handle(name, prec)
        if prec == "single":
            _float_level0(name, dev)
        _check_plan(dev, word, old_word)
        if CASES[name][0] == "scalar":                       # the wider rule admits the scalar level too; "gs+f32" on a block handle names the smoother
            _check_plan(dev, "gs_block+f32", "gs_block")
        else:
            assert "Gauss-Seidel on a block level" in dev.multi_plan(4, fuse="gs+f32")["note"]
        for fuse in (False, True):                           # without the Gauss-Seidel flags: the column loop, as before
            assert dev.multi_plan(4, fuse=fuse)["fused"] == 0 and "level 0" in dev.multi_plan(4, fuse=fuse)["note"], (name, fuse)
    # the double handle: the flag changes nothing
    double = _handle(name, "double")
    for k in (1, 2, 4, 5):
        assert double.multi_plan(k, fuse=word) == double.multi_plan(k, fuse=old_word), (name, k)
        assert double.multi_plan(k, fuse=word)["fused"] == 1, (name, k)


# ---- 2. SmoothMulti against Smooth, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_sweep_equals_the_single_vector_sweep(name):
    _float_level0(name)
    _check_sweeps(_handle(name), _problem(name)[1], _words(name)[1], 3, twin=_handle(name, "wide"))


# ---- scalar kernel coverage: lanes per row x workgroup size, the narrow sweep from zero, no split ------------------------------------------
@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_hybrid_lanes_and_workgroup_sizes(G, threads):
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], "identity")
    env = {"AMGX_GSB_THREADS": str(threads), "AMGX_GSB_THREADS_MULTI": str(threads)}
    single = _dev(H, env, sm_type="hgs", mat_prec="single_gs_all")
    wide = _dev(H, _env(env, WIDE), sm_type="hgs", mat_prec="single_gs_all")
    lp, info = single.level_paths(0), single.gs_prec_info(0)
    assert lp["gs_form"] == "hybrid" and lp["gs_lanes"] == G and lp["gs_threads"] == threads and lp["gs_split"] == 1, lp
    assert info["f32"] == 1 and {"full", "lowin", "rest"} <= set(info["images"]) and single.level_extra(0)["gs_f32"] == 1, info
    _check_plan(single, "gs+f32", "gs")
    _check_sweeps(single, np.asarray(free, dtype=np.float64), "gs+f32", threads + G, twin=wide)
    Bm = np.random.default_rng(G).standard_normal((4, A.shape[0]))
    X = _mult(single, Bm, fuse="gs+f32")
    assert np.array_equal(X, _mult(wide, Bm, fuse="gs+f32")), (G, threads)
    assert np.array_equal(X, _single(single, Bm)), (G, threads, max(_rel(X[j], _single(single, Bm)[j]) for j in range(4)))


@pytest.mark.parametrize("split", [1, 0], ids=["split", "nosplit"])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_hybrid_random_order(G, split):
    """the "random" ordering: mostly off-block couplings, the narrow sweep from zero (with the split); without the split the sweep
    from zero reads `full` and the residual after it the float image of A"""
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], "random")
    env = {} if split else {"AMGX_GSB_NO_SPLIT": "1"}
    single = _dev(H, env, sm_type="hgs", mat_prec="single_gs_all")
    wide = _dev(H, _env(env, WIDE), sm_type="hgs", mat_prec="single_gs_all")
    lp, info = single.level_paths(0), single.gs_prec_info(0)
    assert lp["gs_form"] == "hybrid" and lp["gs_lanes"] == G and lp["gs_split"] == split and info["f32"] == 1, (lp, info)
    if split:
        assert lp["gs_narrow"] == 1, lp
    else:
        assert "A" in info["images"], info
    _check_plan(single, "gs+f32", "gs")
    _check_sweeps(single, np.asarray(free, dtype=np.float64), "gs+f32", 5 * G + split, twin=wide)
    Xf, Cf = single.DownMulti(0, np.ascontiguousarray(np.random.default_rng(G).standard_normal((4, A.shape[0]))), fuse="gs+down+f32")
    Xl, Cl = single.DownMulti(0, np.ascontiguousarray(np.random.default_rng(G).standard_normal((4, A.shape[0]))))
    assert np.array_equal(Xf, Xl) and np.array_equal(Cf, Cl), (G, split)


# ---- 3. MultMulti against Mult, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_cycle_equals_mult(name):
    """k = 2, 4, 5; host arrays and device tensors; captured graph, its replay and direct launches (AMGX_NO_GRAPH).

    Measured on an MI355X (the print of every case): 0 in all 32 cases.  On the block handles that rests on Multi::col_block: with
    the literal multi-vector products around the sweeps a fused column differed from Mult by 1.3e-16 ... 5.4e-16 (on one vector
    Handle::product picks the kernel of a block-CSR matrix per matrix, NV > 1 has one kernel with another order of additions), so the
    transfers and the coarsest solve of such a handle run per column.  The sweeps and the residual after the sweep from zero on BSELL
    images are fused, so this check covers bsell_spmm_kernel<BS, NV, EP_MULT, float> ("hybrid", "hybrid-compact", "bc": r = rest x),
    bgs_bsell_upper_residual_nv_kernel<BS, NV, float> ("mc") and the EP_RES product on the float A (the "-nosplit" forms)."""
    dev = _handle(name)
    _float_level0(name, dev)
    word = _words(name)[1]
    B = np.array(_problem(name)[2])
    one = _single(dev, B)
    assert np.isfinite(one).all() and np.linalg.norm(one) > 0
    worst = 0.0
    got = {}
    for k, interleaved, device, graph in ((2, False, False, True), (4, True, True, True), (5, False, True, False), (4, False, False, False),
                                          (5, True, False, True), (2, True, True, False)):
        assert dev.multi_plan(k, fuse=word)["fused"] == 1
        X = _mult(dev, B[:k], interleaved, device, graph, word)
        got[(k, interleaved, device, graph)] = X
        worst = max(worst, max(_rel(X[j], one[j]) for j in range(k)))
    print(f"{name}: MultMulti against Mult, largest relative difference of a column {worst:.2e}")
    for key, X in got.items():
        k = key[0]
        assert np.array_equal(X, _mult(dev, B[:k], *key[1:], word)), (name, key, "replay")
        assert np.array_equal(X, one[:k]), (name, key, max(_rel(X[j], one[j]) for j in range(k)))


@pytest.mark.parametrize("form,more", [("sell-win", {}), ("sell", {"AMGX_NO_SELL_WINDOW": "1"})])
def test_residual_from_rest_as_a_multi_vector_float_product(form, more):
    """sell_win_spmm_kernel<..., EP_CRES, float> / sell_spmm_kernel<..., EP_CRES, float>: a block-hybrid level with the split whose
    residual after the sweep from zero is NOT fused with the restriction (AMGX_NO_FUSED_RESTRICT), so the fused group runs
    r = c .* x - rest x as one product on NV vectors.  The Kuhn problem and switches of tests/test_gpu_down_family.py; the handle
    created WITH the fused restriction names the format of `rest` on level 0 (level_paths "gs_down"), which the switch does not change."""
    p, H = poisson_case((41, 37, 29), "right|top", 10)
    env = _env(NO_DENSE, {"AMGX_SELL_MAX_LANES": "1"}, more)
    assert _dev(H, env, sm_type="hgs", mat_prec="single_gs_all").level_paths(0)["gs_down"] == form
    env = _env(env, {"AMGX_NO_FUSED_RESTRICT": "1"})
    single = _dev(H, env, sm_type="hgs", mat_prec="single_gs_all")
    wide = _dev(H, _env(env, WIDE), sm_type="hgs", mat_prec="single_gs_all")
    lp, info = single.level_paths(0), single.gs_prec_info(0)
    assert lp["gs_form"] == "hybrid" and lp["gs_split"] == 1 and lp["gs_down"] is None and info["f32"] == 1 and "rest" in info["images"], (lp, info)
    _check_plan(single, "gs+f32", "gs")
    B = np.ascontiguousarray(np.stack([rhs(p, j) for j in range(4)]))
    X, one = _mult(single, B, fuse="gs+f32"), _single(single, B)
    assert np.array_equal(X, one), (form, max(_rel(X[j], one[j]) for j in range(4)))
    assert np.array_equal(X, _mult(wide, B, fuse="gs+f32")), form
    Xd = _mult(_dev(H, env, sm_type="hgs"), B, fuse="gs")
    assert min(_rel(X[j], Xd[j]) for j in range(4)) >= 1e-10, form


# ---- 4. the AMGX_GS_F32_WIDE twin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_wide_twin(name):
    single, wide, double = _handle(name), _handle(name, "wide"), _handle(name, "double")
    _float_level0(name, single)
    word = _words(name)[1]
    B = np.array(_problem(name)[2])
    Xs = _mult(single, B, fuse=word)
    for interleaved, device, graph in ((False, False, True), (True, True, True), (False, True, False)):
        Xw = _mult(wide, B, interleaved, device, graph, word)
        assert np.array_equal(Xs, Xw), (name, interleaved, device, graph, max(_rel(Xs[j], Xw[j]) for j in range(5)))
    Xd = _mult(double, B, fuse=word)
    change = [_rel(Xs[j], Xd[j]) for j in range(4)]          # (the fused columns of both)
    print(f"{name}: fused float against fused double {min(change):.2e} ... {max(change):.2e}")
    assert min(change) >= 1e-10, (name, change)
    assert min(_rel(Xw[j], Xd[j]) for j in range(4)) >= 1e-10, name


# ---- 5. DownMulti ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCALAR)
def test_down_multi(name):
    for prec in ("single", "wide"):
        dev = _handle(name, prec)
        if prec == "single":
            _float_level0(name, dev)
        B = np.array(_problem(name)[2])
        Xl, Cl = dev.DownMulti(0, B)
        for word in ("gs+down+f32", "gs_block+down+f32"):
            Xf, Cf = dev.DownMulti(0, B, fuse=word)
            assert np.array_equal(Xf, Xl) and np.array_equal(Cf, Cl), (name, prec, word)
            Xi, Ci = dev.DownMulti(0, np.ascontiguousarray(B.T), interleaved=True, fuse=word)
            assert np.array_equal(Xi.T, Xl) and np.array_equal(Ci.T, Cl), (name, prec, word, "interleaved")
            plan = dev.multi_level_plan(0, fuse=word)
            assert plan["form"] == "literal" and plan["out"][0] == 0 and plan["note"] == "single-precision Gauss-Seidel images", (name, plan)
        assert not np.array_equal(Xl, _handle(name, "double").DownMulti(0, B)[0]), name


# ---- 6. amgx_pcg_multi ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d-hgs", "b3d-hybrid"])
def test_solve_multi(name):
    from ngsamg_amd.krylov import NativeCGSolver
    H, free, B5 = _problem(name)
    dev = _handle(name)
    _float_level0(name, dev)
    word = _words(name)[1]
    assert dev.multi_plan(4, fuse=word)["fused"] == 1 and dev.multi_plan(4, fuse=word)["groups"] == [4]
    n = dev.sizes[0]
    rng = np.random.default_rng(0)
    B = np.ascontiguousarray(np.stack([B5[0], rng.standard_normal(n) * free, rng.standard_normal(n) * free, np.zeros(n)]))
    tol = 1e-10
    cg = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
    X = np.zeros_like(B)
    cg.SolveMulti(B, X, fuse=word)
    its, errs = cg.iterations, cg.errors
    assert its[3] == 0 and not X[3].any()
    A = H.levels[0].A.to_scipy()
    f = free.astype(bool)
    for j in range(3):
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        print(f"{name} column {j}: iterations multi {its[j]} single {one.iterations}")
        assert its[j] == one.iterations, (j, its[j], one.iterations)
        assert len(errs[j]) == its[j] + 1
        assert np.allclose(errs[j], one.errors, rtol=1e-6, atol=0), j
        assert errs[j][-1] <= tol * errs[j][0], j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j


# ---- 7. mixed handles -------------------------------------------------------------------------------------------------------------------
def test_mixed_handles():
    H, free, B5 = _problem("3d-hgs")
    B = np.array(B5)
    n = H.n_levels
    for prec, want in ((["single_gs_all", "double"] + ["double"] * (n - 2), [0]), (["double", "single_gs_all"] + ["double"] * (n - 2), [1])):
        dev = _dev(H, NO_DENSE, sm_type="hgs", mat_prec=prec)
        assert [l for l in range(n) if dev.gs_prec_info(l)["f32"]] == want, prec
        note = f"single-precision Gauss-Seidel images (level {want[0]})"
        _check_plan(dev, "gs+f32", "gs", note)
        X = _mult(dev, B, fuse="gs+f32")
        one = _single(dev, B)
        print(f"mixed {want}: MultMulti against Mult {max(_rel(X[j], one[j]) for j in range(5)):.2e}")
        assert np.array_equal(X, one), (prec, max(_rel(X[j], one[j]) for j in range(5)))
    # a Gauss-Seidel level above a Chebyshev level with single-precision images
    types = ["hgs", "cheby"] + ["hgs"] * (n - 2)
    lm = [2.5] * n
    # (whether the Chebyshev level gets the float image depends on the format of its A: a small level in CSR-vector form stays fp64)
    dev = _dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm, mat_prec=["single_gs_all", "single"] + ["double"] * (n - 2))
    assert dev.gs_prec_info(0)["f32"] == 1 and dev.smoother_info(1)["sm_type"] == "cheby"
    print("Chebyshev level 1: A", dev.matrix_info(1, "A")["fmt"], "float image", dev.matrix_info(1, "A32")["fmt"])
    _check_plan(dev, "gs+f32", "gs")
    X = _mult(dev, B, fuse="gs+f32")
    one = _single(dev, B)
    print(f"hgs above cheby: MultMulti against Mult {max(_rel(X[j], one[j]) for j in range(5)):.2e}")
    assert np.array_equal(X, one), max(_rel(X[j], one[j]) for j in range(5))
    # single-precision Jacobi images on some level: unfused under every word, with the note it has today
    types = ["hgs", "jacobi"] + ["hgs"] * (n - 2)
    dev = _dev(H, NO_DENSE, sm_type=types, mat_prec=["single_gs_all"] + ["double"] * (n - 1), jacobi_prec=["double", "single"] + ["double"] * (n - 2))
    assert dev.gs_prec_info(0)["f32"] == 1
    for word in ("gs", "gs+f32", "gs_block+f32", "gs+down+f32", True, False):
        plan = dev.multi_plan(4, fuse=word)
        assert plan["fused"] == 0 and plan["groups"] == [1] * 4, (word, plan)
    assert dev.multi_plan(4, fuse="gs+f32")["note"] == "single-precision Jacobi images (level 1)"
    assert dev.multi_plan(4, fuse="gs")["note"] == NOTE
    assert np.array_equal(_mult(dev, B, fuse="gs+f32"), _single(dev, B))


# ---- 8. a level the rule refuses ----------------------------------------------------------------------------------------------------------
def test_formats_without_a_float_image_keep_their_rounded_fp64_values():
    """No switch of the project produces a float level that the rule has to refuse: where `rest` (CSR-vector: a badly padded
    remainder) or A of a level without the split (windowed sliced-ELL, CSR-vector) is stored in a format without a float kernel,
    amgx_create keeps the ROUNDED values at fp64 width (in place / DevMatrix::val64r), the single-vector pass reads that array, and the
    fp64 multi-vector product reads the same one.  So such a level fuses, and this test pins that down: AMGX_SELL_MAX_LANES=1 with and
    without the split on the (17, 17, 17) grid (the formats of tests/test_gpu_mat_prec_sgs.py, DOWN_FORMS); a level that reads float
    images and has no float image of A fuses under "gs+f32" with columns equal to Mult.  The refusal itself (an image without the
    array its single-vector pass reads) is covered by tests/test_multi_f32_cpu.py on the rule."""
    H, free, B5 = _problem("3d-hgs")
    B = np.array(B5)
    seen = set()
    for extra in ({"AMGX_GSB_NO_SPLIT": "1", "AMGX_SELL_MAX_LANES": "1"}, {"AMGX_SELL_MAX_LANES": "1"}, {"AMGX_GSB_NO_SPLIT": "1"}):
        dev = _dev(H, _env(NO_DENSE, extra), sm_type="hgs", mat_prec="single_gs_all")
        lp, info = dev.level_paths(0), dev.gs_prec_info(0)
        assert lp["gs_form"] == "hybrid" and lp["gs_split"] == (0 if "AMGX_GSB_NO_SPLIT" in extra else 1) and info["f32"] == 1, (lp, info)
        for l in range(dev.n_levels - 1):
            if dev.gs_prec_info(l)["f32"]:
                seen.add((dev.level_paths(l)["gs_split"], dev.matrix_info(l, "A")["fmt"], dev.matrix_info(l, "A32")["fmt"]))
        _check_plan(dev, "gs+f32", "gs")
        X, one = _mult(dev, B, fuse="gs+f32"), _single(dev, B)
        assert np.array_equal(X, one), (extra, max(_rel(X[j], one[j]) for j in range(5)))
    print(sorted(seen, key=str))
    assert any(split == 0 and a32 is None for split, a, a32 in seen), seen       # a level whose residual reads val64r of A
