"""Multi-vector apply and PCG (amgx_apply_multi / amgx_matvec_multi / amgx_pcg_multi): k right-hand sides per matrix pass.

Oracle = oracle.pyoracle.Oracle(...).apply / .pcg / .matvec column by column.  Tolerances are the project's:
Jacobi cycles 1e-12 relative, PCG iterations +-1, histories rtol 1e-6, solutions 1e-8, products 1e-13."""
import os

import numpy as np
import pytest

from tests.problems import poisson_case, rhs
from tests.test_gpu_parity import CASES

pytestmark = pytest.mark.gpu

SIZES = CASES + [((25, 25, 25), "right|top", 20)]          # 25^3 has four smoothed levels
GROUPS = {1: [1], 2: [2], 3: [2, 1], 4: [4], 5: [4, 1], 6: [4, 2], 7: [4, 2, 1], 8: [4, 4]}     # fused widths 2 and 4
FMT = {"csrvec": 0, "sell": 1, "sellwin": 3}


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


NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}


def _block(p, k, seed=0):
    return np.stack([rhs(p, seed + j) for j in range(k)])


def _mult(dev, B, interleaved=False, device=False, graph=True, stream=None):
    """X = C B through MultMulti; B and the result are (k, n) whatever the layout handed to the library"""
    Bin = np.ascontiguousarray(B.T) if interleaved else np.ascontiguousarray(B)
    if device:
        import torch
        Bd = torch.from_numpy(Bin).cuda()
        Xd = torch.full_like(Bd, float("nan"))
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                dev.MultMulti(Bd, Xd, interleaved=interleaved, graph=graph)
        else:
            dev.MultMulti(Bd, Xd, interleaved=interleaved, graph=graph)
        torch.cuda.synchronize()
        X = Xd.cpu().numpy()
    else:
        X = np.full_like(Bin, np.nan)
        dev.MultMulti(Bin, X, interleaved=interleaved, graph=graph)
    return np.ascontiguousarray(X.T) if interleaved else X


def _single(dev, B):
    X = np.empty_like(B)
    for j in range(B.shape[0]):
        dev.Mult(np.ascontiguousarray(B[j]), X[j])
    return X


# ---- 1. the fused handle against the oracle's cycle -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,diri,mcs", SIZES)
@pytest.mark.parametrize("env", [None, NO_DENSE], ids=["default", "no_dense_tail"])
def test_fused_cycle_matches_oracle(shape, diri, mcs, env):
    from oracle.pyoracle import Oracle
    p, H = poisson_case(shape, diri, mcs)
    dev = _dev(H, env, sm_type="jacobi")
    B = _block(p, 8, seed=10)
    orc = Oracle(H.levels, sm_type="jacobi")
    ref = np.stack([orc.apply(b) for b in B])
    ci = dev.cycle_info()
    if env is None:
        assert ci["dense_level"] >= 0, ci
    else:
        assert ci["dense_level"] < 0, ci
    for k in range(1, 9):
        info = dev.multi_info(k)
        assert info["fused"] == 1 and info["groups"] == GROUPS[k], (k, info)
        assert info["work_bytes"] > 0 or k == 1
        for interleaved in (False, True):
            for device in (False, True):
                X = _mult(dev, B[:k], interleaved, device)
                for j in range(k):
                    e = _rel(X[j], ref[j])
                    print(f"{shape} {'default' if env is None else 'no_dense_tail'} k={k} il={int(interleaved)} dev={int(device)} col {j}: {e:.2e}")
                    assert e < 1e-12, (k, interleaved, device, j, e)


# ---- 2. every kernel family is exercised by the handles of (1) -------------------------------------------------------------
def test_coverage_of_formats_and_lanes():
    fmts, lanes = set(), set()
    tails = []
    for shape, diri, mcs in SIZES:
        p, H = poisson_case(shape, diri, mcs)
        dev = _dev(H, NO_DENSE, sm_type="jacobi")
        ci = dev.cycle_info()
        tails.append(ci["tail_level"])
        assert ci["dense_level"] < 0
        for l in range(H.n_levels - 1):                     # the levels the multi cycle runs level by level
            for which in ("A", "P", "PT"):
                mi = dev.matrix_info(l, which)
                assert mi["fmt"] in FMT, (shape, l, which, mi)
                fmts.add(FMT[mi["fmt"]])
                if mi["fmt"] == "sell":
                    lanes.add(mi["lanes"])
                print(shape, l, which, mi["fmt"], mi["lanes"])
        dflt = _dev(H, sm_type="jacobi")
        assert dflt.cycle_info()["dense_level"] >= 0
    assert {0, 1, 3} <= fmts, fmts
    assert 1 in lanes and any(g > 1 for g in lanes), lanes
    assert any(t > 0 for t in tails), tails


# ---- 3. k = 1 is the single-vector path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, NO_DENSE], ids=["default", "no_dense_tail"])
def test_k1_is_bit_identical_to_mult(env):
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, env, sm_type="jacobi")
    B = _block(p, 1, seed=3)
    ref = _single(dev, B)
    for interleaved in (False, True):
        for device in (False, True):
            assert np.array_equal(_mult(dev, B, interleaved, device), ref)


# ---- 4. no cross-talk between the columns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, NO_DENSE], ids=["default", "no_dense_tail"])
def test_columns_do_not_talk_to_each_other(env):
    p, H = poisson_case((25, 25, 25), "right|top", 20)
    dev = _dev(H, env, sm_type="jacobi")
    rng = np.random.default_rng(5)
    B8 = _block(p, 8, seed=20)
    X8 = _mult(dev, B8)
    for k in (2, 4, 8):                                      # whole fused groups: all columns of a call take the same kernels
        B = B8[:k]
        X = _mult(dev, B)
        perm = rng.permutation(k)
        while k > 1 and np.array_equal(perm, np.arange(k)):
            perm = rng.permutation(k)
        assert np.array_equal(_mult(dev, B[perm]), X[perm]), k
        assert np.array_equal(_mult(dev, B[perm], interleaved=True, device=True), X[perm]), k
        # a column of NaN leaves the others alone
        Bn = B.copy()
        Bn[k // 2] = np.nan
        Xn = _mult(dev, Bn)
        keep = [j for j in range(k) if j != k // 2]
        assert np.array_equal(Xn[keep], X[keep]), k
        assert np.all(np.isnan(Xn[k // 2][p.free.astype(bool)]))
        # a column's result does not depend on the width it ran at
        for j in range(k):
            e = _rel(X[j], X8[j])
            print(f"width {k} vs 8, column {j}: {e:.2e}")
            assert e < 1e-13, (k, j, e)
    # mixed groups (k = 7 = 4 + 2 + 1): the single column takes the single-vector path
    X7 = _mult(dev, B8[:7])
    assert np.array_equal(X7[6], _single(dev, B8[6:7])[0])
    assert np.array_equal(X7[:4], _mult(dev, B8[:4]))


# ---- 5. graph capture is keyed by k and the layout ------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_graph_replay_with_changing_k_on_the_same_buffers(device):
    import torch
    from oracle.pyoracle import Oracle
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, NO_DENSE, sm_type="jacobi")
    n = p.n
    B = _block(p, 4, seed=30)
    orc = Oracle(H.levels, sm_type="jacobi")
    ref = np.stack([orc.apply(b) for b in B])
    stream = torch.cuda.Stream() if device else None          # (the legacy default stream cannot be captured)
    if device:
        bbuf = torch.from_numpy(B.reshape(-1).copy()).cuda()
        xbuf = torch.empty_like(bbuf)
    else:
        bbuf, xbuf = B.reshape(-1).copy(), np.empty(4 * n)

    def run(k, interleaved, graph):
        src = B[:k].T if interleaved else B[:k]
        shape = (n, k) if interleaved else (k, n)
        if device:
            bbuf[: k * n].copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
            xbuf.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                dev.MultMulti(bbuf[: k * n].view(shape), xbuf[: k * n].view(shape), interleaved=interleaved, graph=graph)
            torch.cuda.synchronize()
            X = xbuf[: k * n].view(shape).cpu().numpy()
        else:
            bbuf[: k * n] = np.ascontiguousarray(src).reshape(-1)
            xbuf[:] = np.nan
            X = xbuf[: k * n].reshape(shape)
            dev.MultMulti(bbuf[: k * n].reshape(shape), X, interleaved=interleaved, graph=graph)
            X = X.copy()
        return np.ascontiguousarray(X.T) if interleaved else X

    got = {}
    for step, (k, il) in enumerate([(4, False), (2, False), (4, False), (4, True), (2, True), (4, False), (3, False), (4, True)]):
        X = run(k, il, True)
        for j in range(k):
            assert _rel(X[j], ref[j]) < 1e-12, (step, k, il, j)
        if (k, il) in got:
            assert np.array_equal(X, got[(k, il)]), (step, k, il)       # the replay
        got[(k, il)] = X
    for (k, il), X in got.items():
        assert np.array_equal(run(k, il, False), X), (k, il)            # direct launches


# ---- 6. every other handle: a column loop over its single-vector path ------------------------------------------------------
def _fallback_handles():
    from ngsamg_amd import fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from tests.problems import elasticity_case
    ps = fem.poisson_fast((21, 21, 21))                       # the problem of smoke()
    Hs = Hierarchy(Matrix(ps.n, ps.n, 1, 1, ps.rowptr, ps.col, ps.val), ps.free, ps.coords, dim=3, energy=0, max_coarse_size=20)
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    pe, He = elasticity_case((13, 11, 9), False, 5, 0.12)
    return [("gs", ps, Hs, dict(sm_type="gs")), ("hgs", ps, Hs, dict(sm_type="hgs")),
            ("W", p, H, dict(sm_type="jacobi", mg_cycle="W")), ("BS", p, H, dict(sm_type="jacobi", mg_cycle="BS")),
            ("steps2", p, H, dict(sm_type="jacobi", sm_steps=2)), ("elasticity", pe, He, dict(sm_type="jacobi"))]


@pytest.mark.parametrize("which", range(6), ids=["gs", "hgs", "W", "BS", "steps2", "elasticity"])
def test_fallback_handles_loop_over_the_single_vector_path(which):
    name, p, H, kw = _fallback_handles()[which]
    dev = _dev(H, **kw)
    rng = np.random.default_rng(which)
    n = dev.sizes[0]
    mask = np.repeat(p.free, p.bs)
    for k in (1, 3, 4):
        info = dev.multi_info(k)
        assert info["fused"] == 0 and info["groups"] == [1] * k, (name, info)
        B = rng.standard_normal((k, n)) * mask
        ref = _single(dev, B)
        assert np.all(np.isfinite(ref))
        for interleaved in (False, True):
            for device in (False, True):
                assert np.array_equal(_mult(dev, B, interleaved, device), ref), (name, k, interleaved, device)
    # the level products take the same loop
    for l in range(dev.n_levels):
        X = rng.standard_normal((3, dev.ext_sizes[l]))
        Y = np.full((3, dev.sizes[l]), np.nan)
        dev.MatVecMulti(l, X, Y)
        for j in range(3):
            y = np.empty(dev.sizes[l])
            dev.MatVec(l, np.ascontiguousarray(X[j]), y)
            assert np.array_equal(Y[j], y), (name, l, j)


# ---- 7. level products ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,diri,mcs", [SIZES[1], SIZES[4]])
def test_matvec_multi_on_every_level(shape, diri, mcs):
    import torch
    from oracle.pyoracle import Oracle
    p, H = poisson_case(shape, diri, mcs)
    dev = _dev(H, NO_DENSE, sm_type="jacobi")
    orc = Oracle(H.levels, sm_type="jacobi")
    rng = np.random.default_rng(7)
    for l in range(H.n_levels):
        n = dev.sizes[l]
        X = rng.standard_normal((8, n))
        ref = np.stack([orc.matvec(l, x) for x in X])
        for k in range(1, 9):
            for interleaved in (False, True):
                Xin = np.ascontiguousarray(X[:k].T) if interleaved else np.ascontiguousarray(X[:k])
                Y = np.full_like(Xin, np.nan)
                dev.MatVecMulti(l, Xin, Y, interleaved=interleaved)
                Yd = torch.full(Xin.shape, float("nan"), dtype=torch.float64, device="cuda")
                dev.MatVecMulti(l, torch.from_numpy(Xin).cuda(), Yd, interleaved=interleaved)
                torch.cuda.synchronize()
                assert np.array_equal(Yd.cpu().numpy(), Y)
                Y = Y.T if interleaved else Y
                for j in range(k):
                    assert _rel(Y[j], ref[j]) < 1e-13, (l, k, interleaved, j, _rel(Y[j], ref[j]))


# ---- 8. k independent CG recurrences ----------------------------------------------------------------------------------------
def _pcg_columns(p):
    rng = np.random.default_rng(0)
    free = p.free.astype(np.float64)
    return np.stack([p.load * free, rng.standard_normal(p.n) * free, rng.standard_normal(p.n) * free, np.zeros(p.n)])


def _check_pcg(p, H, dev, osm, B, X, its, errs, tol):
    from ngsamg_amd.krylov import NativeCGSolver
    from oracle.pyoracle import Oracle
    A = H.levels[0].A.to_scipy()
    f = p.free.astype(bool)
    for j in range(B.shape[0]):
        if not B[j].any():
            assert its[j] == 0 and errs[j] == [0.0]
            continue
        xo, it, eo = Oracle(H.levels, sm_type=osm).pcg(B[j], tol=tol, maxit=100)
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        print(f"column {j}: iterations multi {its[j]}, oracle {it}, single {one.iterations}")
        assert abs(its[j] - it) <= 1 and abs(its[j] - one.iterations) <= 1, (j, its[j], it, one.iterations)
        assert len(errs[j]) == its[j] + 1
        m = min(its[j], it)
        assert np.allclose(errs[j][:m], eo[:m], rtol=1e-6), j
        m = min(its[j], one.iterations)
        assert np.allclose(errs[j][:m], one.errors[:m], rtol=1e-6), j
        assert np.linalg.norm(X[j] - xo) <= 1e-8 * np.linalg.norm(xo), j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["colmajor", "interleaved"])
def test_solve_multi_matches_oracle_pcg(device, interleaved):
    import torch
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = poisson_case((25, 25, 25), "right|top", 20)
    dev = _dev(H, sm_type="jacobi")
    assert dev.multi_info(4)["fused"] == 1
    B = _pcg_columns(p)
    X0 = np.zeros_like(B)                                    # (the zero column starts at err_0 = 0: its x must come back untouched)
    lay = (lambda M: np.ascontiguousarray(M.T)) if interleaved else np.ascontiguousarray
    cg = NativeCGSolver(dev, dev, tol=1e-10, maxsteps=100)
    if device:
        sol = torch.from_numpy(lay(X0)).cuda()
        cg.SolveMulti(torch.from_numpy(lay(B)).cuda(), sol, interleaved=interleaved)
        torch.cuda.synchronize()
        X = sol.cpu().numpy()
    else:
        X = lay(X0)
        cg.SolveMulti(lay(B), X, interleaved=interleaved)
    X = X.T if interleaved else X
    its, errs = cg.iterations, cg.errors
    assert len(its) == 4 and len(errs) == 4
    assert its[3] == 0 and not X[3].any() and not np.signbit(X[3]).any()
    assert its[2] != its[0]                                  # columns stop on their own (oracle: 19, 19, 18 iterations)
    _check_pcg(p, H, dev, "jacobi", B, X, its, errs, 1e-10)
    # the zero column removed: no other column's count changes
    cg3 = NativeCGSolver(dev, dev, tol=1e-10, maxsteps=100)
    cg3.SolveMulti(np.ascontiguousarray(B[:3]))
    assert cg3.iterations == its[:3], (cg3.iterations, its)
    # sol=None starts from zero and returns the solutions
    Xn = NativeCGSolver(dev, dev, tol=1e-10, maxsteps=100).SolveMulti(np.ascontiguousarray(B[:2]))
    assert np.linalg.norm(Xn - X[:2]) <= 1e-8 * np.linalg.norm(X[:2])


def test_solve_multi_without_preconditioner():
    from ngsamg_amd.krylov import NativeCGSolver
    from oracle.pyoracle import Oracle
    p, H = poisson_case((13, 13, 13), "right|top", 20)
    dev = _dev(H, sm_type="jacobi")
    rng = np.random.default_rng(1)
    B = rng.standard_normal((4, p.n)) * p.free
    cg = NativeCGSolver(dev, None, tol=1e-30, maxsteps=15)
    cg.SolveMulti(B)
    orc = Oracle(H.levels, sm_type="jacobi")
    for j in range(4):
        _, it, errs = orc.pcg(B[j], tol=1e-30, maxit=15, precond=False)
        assert cg.iterations[j] == it == 15
        assert np.allclose(cg.errors[j], errs, rtol=1e-8), j


def test_solve_multi_on_a_fallback_handle():
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = poisson_case((25, 25, 25), "right|top", 20)
    dev = _dev(H, sm_type="gs")
    assert dev.multi_info(4)["fused"] == 0
    B = _pcg_columns(p)
    X = np.zeros_like(B)
    cg = NativeCGSolver(dev, dev, tol=1e-10, maxsteps=100)
    cg.SolveMulti(B, X)
    assert cg.iterations[3] == 0 and not X[3].any()
    _check_pcg(p, H, dev, "gs_mc", B, X, cg.iterations, cg.errors, 1e-10)


# ---- argument errors reach the caller as NgsAMGError -------------------------------------------------------------------------
def test_native_argument_errors():
    import ctypes as C
    from ngsamg_amd._lib import NgsAMGError
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, sm_type="jacobi")
    n = p.n
    b, x = np.ones((2, n)), np.zeros((2, n))
    lib = dev._lib
    assert lib.amgx_apply_multi(dev._h, 9, b.ctypes.data, n, x.ctypes.data, n, 0, 0) != 0
    assert "k must be 1 .. 8" in lib.amgx_last_error(dev._h).decode()
    assert lib.amgx_apply_multi(dev._h, 0, b.ctypes.data, n, x.ctypes.data, n, 0, 0) != 0
    assert lib.amgx_apply_multi(dev._h, 2, b.ctypes.data, n - 1, x.ctypes.data, n, 0, 0) != 0
    assert "leading dimension" in lib.amgx_last_error(dev._h).decode()
    assert lib.amgx_apply_multi(dev._h, 2, b.ctypes.data, n, b.ctypes.data, n, 0, 0) != 0
    assert lib.amgx_matvec_multi(dev._h, 99, 2, b.ctypes.data, n, x.ctypes.data, n, 0) != 0
    assert lib.amgx_multi_info(dev._h, 9, None, None, None, None) != 0
    with pytest.raises(NgsAMGError):
        dev.multi_info(0)
    with pytest.raises(NgsAMGError):
        dev.MultMulti(np.ones((9, n)), np.zeros((9, n)))
    # a leading dimension larger than n (host, column-major): the columns in between stay untouched
    ld = n + 5
    Bp, Xp = np.zeros((2, ld)), np.full((2, ld), -3.0)
    Bp[:, :n] = _block(p, 2, seed=40)
    assert lib.amgx_apply_multi(dev._h, 2, Bp.ctypes.data, ld, Xp.ctypes.data, ld, 0, 0) == 0
    assert np.all(Xp[:, n:] == -3.0)
    assert np.array_equal(Xp[:, :n], _mult(dev, np.ascontiguousarray(Bp[:, :n])))
    assert C.sizeof(C.c_int64) == 8


# ---- a leading dimension above the level size, k = 7 (groups 4 + 2 + 1) and k = 4, host arrays and device tensors -------------------
@pytest.mark.parametrize("sm", ["jacobi", "gs"])        # fused groups; the column loop over the single-vector path
def test_column_major_with_a_leading_dimension_above_n(sm):
    from tests.problems import padded_call
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, NO_DENSE, sm_type=sm)
    assert dev.multi_info(7)["groups"] == ([4, 2, 1] if sm == "jacobi" else [1] * 7)
    lib, h = dev._lib, dev._h
    B = _block(p, 7, seed=60)
    ref = _mult(dev, B)                                  # the same call with ld = n
    if sm == "gs":
        assert np.array_equal(ref, _single(dev, B))
    rng = np.random.default_rng(61)
    for k in (7, 4):
        for device in (False, True):
            def apply(kk, a, flags):
                assert lib.amgx_apply_multi(h, kk, a[0][0], a[0][1], a[1][0], a[1][1], 0, flags) == 0, lib.amgx_last_error(h)
            _, X = padded_call(dev, apply, [B[:k], np.full((k, p.n), np.nan)], device)
            assert np.array_equal(X, ref[:k]), (sm, k, device)
            for l in range(2):
                V = rng.standard_normal((k, dev.ext_sizes[l]))
                want = np.empty((k, dev.sizes[l]))
                for j in range(k):
                    dev.MatVec(l, np.ascontiguousarray(V[j]), want[j])

                def matvec(kk, a, flags):
                    assert lib.amgx_matvec_multi(h, l, kk, a[0][0], a[0][1], a[1][0], a[1][1], flags) == 0, lib.amgx_last_error(h)
                Vout, Y = padded_call(dev, matvec, [V, np.full((k, dev.sizes[l]), np.nan)], device)
                assert np.array_equal(Vout, V)
                Yw = np.full((k, dev.sizes[l]), np.nan)
                dev.MatVecMulti(l, V, Yw)                # ld = n
                assert np.array_equal(Y, Yw), (sm, k, device, l)
                if sm == "gs":                           # the column loop: amgx_matvec itself
                    assert np.array_equal(Y, want), (sm, k, device, l)
                else:
                    assert max(_rel(Y[j], want[j]) for j in range(k)) < 1e-13, (sm, k, device, l)
