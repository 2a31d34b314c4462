"""AMGX_MULTI_FUSE_GS (fuse="gs"): fused multi-vector cycles on scalar Gauss-Seidel levels, block-hybrid and
multicolour form.

References: the single-vector sweep of the same handle (bit for bit, through SmoothMulti / Smooth), oracle.pyoracle.Oracle with
tests.hgs_oracle.hgs_levels (the bound of tests/test_gpu_hgs.py: 1e-10 relative), Mult of the same handle (1e-12: the single-vector
down pass restricts chunk-locally, another summation order in P^T r).  PCG: iterations +-1, histories rtol 1e-6, residuals 1e-8."""
import functools
import os

import numpy as np
import pytest

from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, env=None, **kw):
    """DeviceAMGMatrix created with `env` set in os.environ (restored afterwards: the switches are read by amgx_create)"""
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


SHAPES = {"21": (21, 21, 21), "33": (33, 30, 28), "70": (70, 70), "40": (40, 38, 30)}

# handle specifications: name -> (shape, smoother, environment)
SPECS = {
    "21-hgs": ("21", "hgs", {}),                                             # 36 blocks of 256 rows plus a partial one; dense tail
    "21-hgs-levels": ("21", "hgs", NO_DENSE),                                # ... the small levels really sweep
    "33-hgs-levels": ("33", "hgs", NO_DENSE),                                # coarse levels with G > 1 lanes per row
    "70-hgs-levels": ("70", "hgs", NO_DENSE),                                # 2-D: short rows, narrow `lowin`
    "21-hgs-512": ("21", "hgs", dict(NO_DENSE, AMGX_GSB_THREADS="512")),
    "33-hgs-1024": ("33", "hgs", dict(NO_DENSE, AMGX_GSB_THREADS="1024")),
    "21-hgs-nosplit": ("21", "hgs", dict(NO_DENSE, AMGX_GSB_NO_SPLIT="1")),   # the sweep from zero on `full`, EP_RES on A
    "21-gs-levels": ("21", "gs", NO_DENSE),                                  # multicolour form
    "33-gs": ("33", "gs", {}),
    "21-mixed": ("21", "mixed", NO_DENSE),                                   # hgs on level 0, Jacobi below
}
ALL = list(SPECS)
# (the sweep test only) the local-window image of the general single-vector sweep, forced onto the small coarse levels
SPECS["40-hgs-lw"] = ("40", "hgs", dict(NO_DENSE, AMGX_LW_MIN_ROWS="300", AMGX_GSB_LW="1"))
SWEEP = ALL + ["40-hgs-lw"]


def _problem(name):
    return poisson_case(SHAPES[SPECS[name][0]], "right|top", 20)


def _handle(name, **more):
    shape, sm, env = SPECS[name]
    H = _problem(name)[1]
    if sm == "mixed":
        sm = ["hgs"] + ["jacobi"] * (H.n_levels - 1)
    return _dev(H, env, sm_type=sm, **more)


def _smoothed(dev):
    return range(dev.n_levels - 1)


def _check_forms(name, dev):
    """the handle really is the case its name says (a hierarchy that does not produce the form is a wrong case)"""
    shape, sm, env = SPECS[name]
    lp = [dev.level_paths(l) for l in _smoothed(dev)]
    forms = [p["gs_form"] for p in lp]
    if sm == "hgs":
        assert forms[0] == "hybrid" and set(forms) <= {"hybrid", "mc"}, (name, forms)
        if "AMGX_GSB_THREADS" in env:
            assert lp[0]["gs_threads"] == int(env["AMGX_GSB_THREADS"]), (name, lp[0])
        elif shape == "21":
            assert lp[0]["gs_threads"] == 256 and lp[0]["gs_lanes"] == 1, (name, lp[0])
        assert lp[0]["gs_split"] == (0 if "AMGX_GSB_NO_SPLIT" in env else 1), (name, lp[0])
        if shape == "33":
            # coarse levels with several lanes per row: the narrow sweep from zero, the mid-width general sweep, and a multicolour tail
            multi = [p for p in lp if p["gs_form"] == "hybrid" and p["gs_lanes"] > 1]
            assert multi and any(p["gs_narrow"] for p in multi) and any(p["gs_mid"] for p in multi), (name, multi)
            assert any(not p["gs_mid"] for p in multi) and forms[-1] == "mc", (name, multi, forms)
        if shape == "70":
            assert lp[0]["gs_full_maxw"] <= 7 and lp[0]["gs_lowin_maxw"] <= 6 and not lp[0]["gs_narrow"], (name, lp[0])
    elif sm == "gs":
        assert set(forms) == {"mc"}, (name, forms)
    else:
        assert forms[0] == "hybrid" and set(forms[1:]) <= {None}, (name, forms)
        assert [dev.smoother_info(l)["sm_type"] for l in _smoothed(dev)] == ["gs"] + ["jacobi"] * (dev.n_levels - 2)
    if env.get("AMGX_NO_DENSE_TAIL"):
        assert dev.cycle_info()["dense_level"] < 0, name
    return lp


@functools.lru_cache(maxsize=None)
def _block(name, k=8, seed=0):
    p = _problem(name)[0]
    B = np.stack([rhs(p, seed + j) for j in range(k)])
    B.setflags(write=False)
    return B


_ORACLE = {}


def _reference(name, dev):
    """the oracle's cycle on the 8 columns of _block(name), computed once per (shape, smoother): the hybrid oracle is configured
    with the blocks, colours and diagonal the handle was created with (tests.hgs_oracle), which the variants of a shape share
    unless the workgroup size changes the blocks"""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    shape, sm, env = SPECS[name]
    key = (shape, sm, env.get("AMGX_GSB_THREADS"))
    if key not in _ORACLE:
        H = _problem(name)[1]
        if sm == "gs":
            orc = Oracle(H.levels, sm_type="gs_mc")
        else:
            lv, types = hgs_levels(H.levels, dev.hgs)
            if sm == "mixed":
                types = [types[0]] + ["jacobi"] * (len(types) - 1)
            orc = Oracle(lv, sm_type=types)
        X = np.stack([orc.apply(np.array(b)) for b in _block(name)])
        X.setflags(write=False)
        _ORACLE[key] = X
    return _ORACLE[key]


def _mult(dev, B, interleaved=False, device=False, graph=True, fuse="gs"):
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


def _check_plan(k, plan):
    assert plan["fused"] == 1 and plan["note"] == "", (k, plan)
    assert sum(plan["groups"]) == k and set(plan["groups"]) <= {1, 2, 4}, (k, plan)
    if k >= 2:
        assert max(plan["groups"]) >= 2, plan
    assert plan["work_bytes"] > 0 or k == 1, (k, plan)


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_plan(name):
    dev = _handle(name)
    _check_forms(name, dev)
    for k in range(1, 9):
        _check_plan(k, dev.multi_plan(k, fuse="gs"))
        info = dev.multi_info(k)
        for fuse in (True, False):                     # without the new bit: what the handle answers today
            plan = dev.multi_plan(k, fuse=fuse)
            assert plan["fused"] == 0 and plan["groups"] == [1] * k, (name, k, fuse, plan)
            assert "smoother" in plan["note"] and "level 0" in plan["note"], (name, k, fuse, plan)
            assert {key: plan[key] for key in info} == info, (name, k, fuse, plan, info)


def test_plan_of_a_block_level_handle_keeps_the_column_loop():
    p, H = elasticity_case((9, 8, 7), False, 5, 0.12)
    dev = _dev(H, sm_type="hgs")
    for k in (1, 3, 4, 8):
        plan = dev.multi_plan(k, fuse="gs")
        assert plan["fused"] == 0 and plan["groups"] == [1] * k, plan
        assert "Gauss-Seidel on a block level" in plan["note"] and "level 0" in plan["note"], plan
    B = np.stack([rhs(p, j) for j in range(3)])
    assert np.array_equal(_mult(dev, B, fuse="gs"), _single(dev, B))       # the flag is never an error


# ---- 2. sweep against sweep, bit for bit ------------------------------------------------------------------------------------

def _smooth_multi(dev, level, X0, B, x_zero, back, interleaved, device):
    Xin = np.array(X0.T if interleaved else X0, order="C")
    Bin = np.array(B.T if interleaved else B, order="C")
    if device:
        import torch
        Xd, Bd = torch.from_numpy(Xin).cuda(), torch.from_numpy(Bin).cuda()
        dev.SmoothMulti(level, Xd, Bd, x_zero=x_zero, back=back, interleaved=interleaved, fuse="gs")
        torch.cuda.synchronize()
        Xin = Xd.cpu().numpy()
    else:
        dev.SmoothMulti(level, Xin, Bin, x_zero=x_zero, back=back, interleaved=interleaved, fuse="gs")
    return np.ascontiguousarray(Xin.T) if interleaved else Xin


@pytest.mark.parametrize("name", SWEEP)
def test_sweep_equals_the_single_vector_sweep(name):
    dev = _handle(name)
    lp = _check_forms(name, dev) if name in ALL else [dev.level_paths(l) for l in _smoothed(dev)]
    if name == "40-hgs-lw":
        assert any(p["gs_lw"] == 1 for p in lp), [(p["gs_form"], p["gs_lanes"], p["gs_lw"]) for p in lp]
    rng = np.random.default_rng(3)
    seen = set()
    for level in _smoothed(dev):
        n = dev.sizes[level]
        free = _problem(name)[1].levels[level].free.astype(np.float64)
        B = rng.standard_normal((7, n)) * free
        Xs = rng.standard_normal((7, n)) * free
        seen.add((lp[level]["gs_form"], lp[level]["gs_lanes"] > 1, lp[level]["gs_mid"], lp[level]["gs_lw"]))
        for back in (False, True):
            for x_zero in (False, True):
                X0 = np.zeros_like(Xs) if x_zero else Xs
                one = X0.copy()
                for j in range(7):
                    dev.Smooth(level, one[j], np.ascontiguousarray(B[j]), np.zeros(n), x_zero=x_zero, back=back)
                assert not np.array_equal(one, X0)
                for k in (2, 4, 7):
                    for interleaved in (False, True):
                        for device in (False, True):
                            X = _smooth_multi(dev, level, X0[:k], B[:k], x_zero, back, interleaved, device)
                            assert np.array_equal(X, one[:k]), (name, level, back, x_zero, k, interleaved, device,
                                                                float(np.abs(X - one[:k]).max()))
    print(name, sorted(seen, key=str))


# ---- 3. / 4. the cycle against the oracle and against Mult --------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_cycle_matches_oracle_and_mult(name):
    dev = _handle(name)
    _check_forms(name, dev)
    B, ref = _block(name), _reference(name, dev)
    one = _single(dev, np.array(B))
    worst = em = 0.0
    for k, interleaved, device, graph in ((8, False, False, True), (2, True, True, True), (7, False, True, False), (4, True, False, True),
                                          (3, False, False, True), (6, True, True, False)):
        _check_plan(k, dev.multi_plan(k, fuse="gs"))
        X = _mult(dev, B[:k], interleaved, device, graph)
        for j in range(k):
            e, m = _rel(X[j], ref[j]), _rel(X[j], one[j])
            worst, em = max(worst, e), max(em, m)
            assert e <= 1e-10, (name, k, interleaved, device, graph, j, e)
            assert m <= 1e-12, (name, k, interleaved, device, graph, j, m)
        if k in (7, 3):
            assert np.array_equal(X[k - 1], one[k - 1]), (name, k)      # the single column IS the single-vector path
    print(f"{name}: vs oracle {worst:.2e} (1e-10), vs Mult {em:.2e} (1e-12)")


# ---- 5. no cross-talk between the columns -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33-hgs-levels", "21-hgs", "21-gs-levels", "21-mixed"])
def test_columns_do_not_talk_to_each_other(name):
    p = _problem(name)[0]
    dev = _handle(name)
    free = np.repeat(p.free, p.bs).astype(bool)
    rng = np.random.default_rng(5)
    B8 = np.array(_block(name, seed=20))
    X8 = _mult(dev, B8)
    for k in (2, 4, 8):
        B = B8[:k]
        X = _mult(dev, B)
        perm = rng.permutation(k)
        while np.array_equal(perm, np.arange(k)):
            perm = rng.permutation(k)
        assert np.array_equal(_mult(dev, B[perm]), X[perm]), k
        assert np.array_equal(_mult(dev, B[perm], interleaved=True, device=True), X[perm]), k
        Bn = B.copy()
        Bn[k // 2] = np.nan
        Xn = _mult(dev, Bn)
        keep = [j for j in range(k) if j != k // 2]
        assert np.array_equal(Xn[keep], X[keep]), k
        assert np.all(np.isnan(Xn[k // 2][free])), k
        assert np.array_equal(X, X8[:k]), k                     # a column's bits do not depend on the width of its group
    # k = 1 with the flag is the single-vector path itself; so is the single column of k = 7 = 4 + 2 + 1
    assert np.array_equal(_mult(dev, B8[:1]), _single(dev, B8[:1]))
    assert np.array_equal(_mult(dev, B8[:1], interleaved=True, device=True), _single(dev, B8[:1]))
    X7 = _mult(dev, B8[:7])
    assert np.array_equal(X7[6], _single(dev, B8[6:7])[0])
    assert np.array_equal(X7[:4], _mult(dev, B8[:4]))


# ---- 6. graphs are keyed by k, the layout and the rule ----------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["21-hgs-levels", "21-gs-levels"])
def test_graph_replay_with_changing_k_and_flag_on_the_same_buffers(name, device):
    import torch
    dev = _handle(name)
    n = dev.sizes[0]
    B = np.array(_block(name)[:4])
    fresh = {fuse: _mult(_handle(name), B, fuse=fuse) for fuse in ("gs", True, False)}
    loop = _single(_handle(name), B)
    assert np.array_equal(fresh[True], loop) and np.array_equal(fresh[False], loop)
    stream = torch.cuda.Stream() if device else None          # (the legacy default stream cannot be captured)
    if device:
        bbuf = torch.from_numpy(B.reshape(-1).copy()).cuda()
        xbuf = torch.empty_like(bbuf)
    else:
        bbuf, xbuf = B.reshape(-1).copy(), np.empty(4 * n)

    def run(k, interleaved, fuse, graph=True):
        src = B[:k].T if interleaved else B[:k]
        shape = (n, k) if interleaved else (k, n)
        if device:
            bbuf[: k * n].copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
            xbuf.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                dev.MultMulti(bbuf[: k * n].view(shape), xbuf[: k * n].view(shape), interleaved=interleaved, graph=graph, fuse=fuse)
            torch.cuda.synchronize()
            X = xbuf[: k * n].view(shape).cpu().numpy()
        else:
            bbuf[: k * n] = np.ascontiguousarray(src).reshape(-1)
            xbuf[:] = np.nan
            X = xbuf[: k * n].reshape(shape)
            dev.MultMulti(bbuf[: k * n].reshape(shape), X, interleaved=interleaved, graph=graph, fuse=fuse)
            X = X.copy()
        return np.ascontiguousarray(X.T) if interleaved else X

    got = {}
    steps = [(4, False, "gs"), (2, False, "gs"), (4, False, False), (4, False, "gs"), (4, True, "gs"), (2, True, True), (2, True, "gs"),
             (4, False, True), (3, False, "gs"), (4, True, "gs"), (3, False, False), (4, False, "gs")]
    for step, (k, il, fuse) in enumerate(steps):
        X = run(k, il, fuse)
        # the results of fresh handles: the fused groups' bits do not depend on k (check 5), the column loop is Mult
        want = fresh[fuse][:k].copy()
        if fuse == "gs" and k == 3:
            want[2] = loop[2]
        assert np.array_equal(X, want), (step, k, il, fuse)
        got[(k, il, fuse)] = X
    for (k, il, fuse), X in got.items():
        assert np.array_equal(run(k, il, fuse, graph=False), X), (k, il, fuse)   # direct launches


# ---- 7. k independent CG recurrences ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_solve_multi(device):
    import torch
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = _problem("21-hgs")
    dev = _handle("21-hgs")
    assert dev.multi_plan(4, fuse="gs")["fused"] == 1 and dev.multi_plan(4, fuse="gs")["groups"] == [4]
    n = dev.sizes[0]
    free = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    B = np.stack([np.asarray(p.load, dtype=np.float64).reshape(-1) * free, rng.standard_normal(n) * free, rng.standard_normal(n) * free,
                  np.zeros(n)])
    interleaved = device
    lay = (lambda M: np.ascontiguousarray(M.T)) if interleaved else np.ascontiguousarray
    tol = 1e-10
    cg = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
    if device:
        sol = torch.from_numpy(lay(np.zeros_like(B))).cuda()
        cg.SolveMulti(torch.from_numpy(lay(B)).cuda(), sol, interleaved=interleaved, fuse="gs")
        torch.cuda.synchronize()
        X = sol.cpu().numpy()
    else:
        X = lay(np.zeros_like(B))
        cg.SolveMulti(lay(B), X, interleaved=interleaved, fuse="gs")
    X = X.T if interleaved else X
    its, errs = cg.iterations, cg.errors
    assert its[3] == 0 and errs[3] == [0.0] and not X[3].any() and not np.signbit(X[3]).any()
    A = H.levels[0].A.to_scipy()
    f = free.astype(bool)
    for j in range(3):
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        print(f"column {j}: iterations multi {its[j]} single {one.iterations}")
        assert abs(its[j] - one.iterations) <= 1, (j, its[j], one.iterations)
        assert len(errs[j]) == its[j] + 1
        m = min(its[j], one.iterations)
        assert np.allclose(errs[j][:m], one.errors[:m], rtol=1e-6, atol=0), j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j


# ---- 8. the fused cycle is symmetric ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33-hgs-levels", "21-hgs", "21-gs-levels", "21-mixed"])
def test_fused_cycle_is_symmetric(name):
    dev = _handle(name)
    B = np.array(_block(name, seed=40)[:4])
    X = _mult(dev, B, interleaved=True, device=True)
    for u, v in ((0, 1), (2, 3)):
        a, b = float(B[v] @ X[u]), float(B[u] @ X[v])           # v^T C u and u^T C v from one fused call
        assert abs(a - b) <= 1e-10 * abs(a), (name, u, v, a, b)


# ---- a leading dimension above the level size: k = 7 (groups 4 + 2 + 1) and k = 4, host arrays and device tensors -------------------
def test_sweep_with_a_leading_dimension_above_n():
    from ngsamg_amd import _lib
    from tests.problems import padded_call
    name, level = "21-hgs-levels", 0
    dev = _handle(name)
    lib, h = dev._lib, dev._h
    n = dev.sizes[level]
    free = _problem(name)[1].levels[level].free.astype(np.float64)
    rng = np.random.default_rng(5)
    B, X0 = rng.standard_normal((7, n)) * free, rng.standard_normal((7, n)) * free
    for back in (False, True):
        one = X0.copy()
        for j in range(7):
            dev.Smooth(level, one[j], np.ascontiguousarray(B[j]), np.zeros(n), back=back)
        for flag in (0, _lib.AMGX_MULTI_FUSE | _lib.AMGX_MULTI_FUSE_GS):      # the column loop and the multi-vector sweeps
            for k in (7, 4):
                for device in (False, True):
                    def smooth(kk, a, flags):
                        rc = lib.amgx_smooth_multi(h, level, int(back), kk, a[0][0], a[0][1], a[1][0], a[1][1], 0, flags | flag)
                        assert rc == 0, lib.amgx_last_error(h)
                    X, Bout = padded_call(dev, smooth, [X0[:k], B[:k]], device)
                    assert np.array_equal(Bout, B[:k])
                    assert np.array_equal(X, one[:k]), (back, flag, k, device, float(np.abs(X - one[:k]).max()))
