"""The native single-GPU Krylov solvers (amgx_pcg, its single-reduction form, amgx_gmres, amgx_pcg_multi) where
tests/test_gpu_krylov.py does not go: exact reductions at the boundaries of their three regimes, initial guesses, block systems,
the documented argument edges and the work space the solvers share inside a handle.

References: the CPU oracle's pcg / gmres (pinned by tests/test_krylov_cpu.py) and exact integer arithmetic.  Tolerances are the
existing ones (tests/test_gpu_krylov.py, tests/test_gpu_multi_rhs.py): PCG iterations +-1, histories rtol 1e-6, solutions 1e-8;
GMRES same count, history to 1e-6 err_0, first four entries rtol 1e-9, solutions 1e-7; plain CG histories rtol 1e-8."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests.krylov_cases import (EDGE_SHAPES, device_handle, edge_case, elasticity3, elasticity6, exact_norm, free_mask, fsum_norm2, guess,
                                integer_vectors, native_solve, native_solve_multi, rel)
from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

OSM = {"jacobi": "jacobi", "gs": "gs_mc"}          # the device's multicolour Gauss-Seidel = the oracle's sweep in colour-major order
EDGE_IDS = ["x".join(map(str, s)) for s in EDGE_SHAPES]


@functools.lru_cache(maxsize=None)
def _edge_dev(shape, sm="jacobi"):
    p, H = edge_case(shape)
    return p, H, device_handle(H, sm_type=sm)


@functools.lru_cache(maxsize=None)
def _p25(sm):
    p, H = poisson_case((25, 25, 25), "right|top", 20)
    return p, H, device_handle(H, sm_type=sm)


@functools.lru_cache(maxsize=None)
def _oracle(case, osm, cycle="V"):
    from oracle.pyoracle import Oracle
    return Oracle(case()[1].levels, sm_type=osm, cycle=cycle)


def _case25():
    return poisson_case((25, 25, 25), "right|top", 20)


def _case17():
    return poisson_case((17, 17, 17), "right|top", 20)


def _check_pcg(got, ref, tol, tag=""):
    x, it, errs = got
    xo, ito, erro = ref
    k = min(it, ito)
    print(f"{tag}: it {it} / {ito}, history {np.max(np.abs(errs[:k] - erro[:k]) / erro[:k]) if k else 0.0:.2e}, solution {rel(x, xo):.2e}")
    assert abs(it - ito) <= 1, (tag, it, ito)
    assert errs.size == it + 1 and np.all(np.isfinite(errs))
    assert np.allclose(errs[:k], erro[:k], rtol=1e-6, atol=0), tag
    # one iteration more or less moves the solution by the order of the stopping tolerance
    assert rel(x, xo) <= (1e-8 if it == ito else max(1e-8, 100 * tol)), tag


def _check_gmres(got, ref, tag="", slack=0):
    x, it, errs = got
    xo, ito, erro = ref
    k = min(it, ito) + 1
    print(f"{tag}: it {it} / {ito}, history {np.max(np.abs(errs[:k] - erro[:k])) / erro[0]:.2e} err_0, solution {rel(x, xo):.2e}")
    assert abs(it - ito) <= slack, (tag, it, ito)
    assert errs.size == it + 1 and np.all(np.abs(errs[:k] - erro[:k]) <= 1e-6 * erro[0]), tag
    assert np.allclose(errs[:4], erro[:4], rtol=1e-9, atol=0), tag
    assert rel(x, xo) <= 1e-7, tag


# ---- a. exact reductions at the regime boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=EDGE_IDS)
def test_first_history_entry_is_the_exact_norm_of_an_integer_rhs(shape):
    """use_precond = 0, x = 0: err_0 = sqrt(<b, b>) through the residual kernel and ONE reduction.  Integer entries make every
    partial sum exact, so the value does not depend on the order of the additions: bitwise equality with the integer result.
    amgx_pcg: kr_dot_kernel; amgx_gmres: the same kernel on (V, V)."""
    p, H, dev = _edge_dev(shape)
    n = p.n
    for name, b in integer_vectors(n, seed=n):
        want = exact_norm(b)
        for device_vectors in (False, True):
            x, it, errs = native_solve(dev, "pcg", b, maxit=0, pre=False, device_vectors=device_vectors)
            assert it == 0 and errs.tolist() == [want], ("pcg", shape, name, device_vectors, errs, want)
            assert not x.any()
            # tol = 2: GMRES stops before its first iteration with err_0 = |b| written
            x, it, errs = native_solve(dev, "gmres", b, tol=2.0, maxit=1, restart=5, pre=False, device_vectors=device_vectors)
            assert it == 0 and errs.tolist() == [want], ("gmres", shape, name, device_vectors, errs, want)
            assert not x.any()


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=EDGE_IDS)
def test_multi_first_history_entries_are_exact_for_integer_columns(shape):
    """amgx_pcg_multi, k = 1 .. 8 distinct integer columns, both layouts: kr_dot_multi_partial_kernel + kr_dot_final_kernel"""
    p, H, dev = _edge_dev(shape)
    n = p.n
    vecs = integer_vectors(n, seed=n + 1)
    last = np.zeros(n)
    last[n - 1] = 5.0
    cols = [vecs[0][1], last] + [np.random.default_rng(100 * n + j).integers(-8, 9, size=n).astype(np.float64) for j in range(6)]
    for k in range(1, 9):
        B = np.stack(cols[:k])
        want = [exact_norm(c) for c in cols[:k]]
        for interleaved in (False, True):
            for device_vectors in ((False, True) if k in (1, 4, 7) else (True,)):
                X, its, errs = native_solve_multi(dev, B, maxit=0, pre=False, interleaved=interleaved, device_vectors=device_vectors)
                assert its == [0] * k and [e.tolist() for e in errs] == [[w] for w in want], (shape, k, interleaved, device_vectors, errs, want)
                assert not X.any()


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=EDGE_IDS)
def test_first_history_entry_for_generic_data(shape):
    """standard_normal data against the sum of long-double products by math.fsum.  All terms are non-negative, so any order of
    the n additions stays within n 2^-53 of the exact sum (loose on purpose: the integer cases are the sharp ones)."""
    p, H, dev = _edge_dev(shape)
    n = p.n
    B = np.random.default_rng(n).standard_normal((3, n))
    for j in range(2):
        s_exact = fsum_norm2(B[j])
        for kind, kw in (("pcg", dict(maxit=0)), ("gmres", dict(tol=2.0, maxit=1, restart=5))):
            _, _, errs = native_solve(dev, kind, B[j], pre=False, **kw)
            s = errs[0] ** 2
            print(f"{shape} {kind}: |s - s_exact| / s_exact = {abs(s - s_exact) / s_exact:.2e} (bound {n * 2.0 ** -53:.2e})")
            assert abs(s - s_exact) <= n * 2.0 ** -53 * s_exact, (shape, kind)
    for interleaved in (False, True):
        _, _, errs = native_solve_multi(dev, B, maxit=0, pre=False, interleaved=interleaved)
        for j in range(3):
            s_exact = fsum_norm2(B[j])
            assert abs(errs[j][0] ** 2 - s_exact) <= n * 2.0 ** -53 * s_exact, (shape, interleaved, j)


# ---- b. histories at the size edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=EDGE_IDS)
def test_plain_cg_history_at_the_size_edges(shape):
    """use_precond = 0 against Oracle.pcg(precond=False), iteration by iteration.  maxit stays below the number of free dofs
    ((3,3) has 4): beyond it the recurrence divides 0 by 0 in the reference too."""
    from oracle.pyoracle import Oracle
    p, H, dev = _edge_dev(shape)
    nfree = int(np.count_nonzero(p.free))
    maxit = min(15, nfree - 1)
    b = rhs(p, 1)
    _, ito, erro = Oracle(H.levels, sm_type="jacobi").pcg(b, tol=1e-30, maxit=maxit, precond=False)
    for device_vectors in (True, False):
        _, it, errs = native_solve(dev, "pcg", b, tol=1e-30, maxit=maxit, pre=False, device_vectors=device_vectors)
        print(f"{shape} free {nfree}: {maxit} iterations, history {np.max(np.abs(errs - erro) / erro):.2e}")
        assert it == ito == maxit
        assert np.allclose(errs, erro, rtol=1e-8, atol=0)
    # the k recurrences of amgx_pcg_multi are this recurrence per column
    B = np.stack([b, rhs(p, 2), rhs(p, 3)])
    X, its, errs = native_solve_multi(dev, B, tol=1e-30, maxit=maxit, pre=False, interleaved=True)
    assert its == [maxit] * 3 and np.allclose(errs[0], erro, rtol=1e-8, atol=0)


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
@pytest.mark.parametrize("shape", [(7, 9), (5, 13), (16, 16), (65, 65, 63)], ids=["7x9", "5x13", "16x16", "65x65x63"])
def test_preconditioned_solvers_at_the_size_edges(shape, sm):
    """PCG, single-reduction PCG and GMRES(5) at 63, 65, 256 and 266 175 unknowns.  Systems with fewer than 50 free dofs stop at
    1e-6, before finite termination turns the tail of the history into rounding noise."""
    from oracle.pyoracle import Oracle
    p, H, dev = _edge_dev(shape, sm)
    tol = 1e-6 if np.count_nonzero(p.free) < 50 else 1e-10
    b = rhs(p, 1)
    orc = Oracle(H.levels, sm_type=OSM[sm])
    ref = orc.pcg(b, tol=tol, maxit=100)
    assert ref[1] < 100
    _check_pcg(native_solve(dev, "pcg", b, tol=tol, maxit=100), ref, tol, f"{shape} {sm} pcg")
    _check_pcg(native_solve(dev, "pcg_sr", b, tol=tol, maxit=100), ref, tol, f"{shape} {sm} pcg_sr")
    gtol = 1e-6 if tol == 1e-6 else 1e-9
    refg = orc.gmres(b, tol=gtol, maxit=150, restart=5)
    assert refg[1] < 150
    _check_gmres(native_solve(dev, "gmres", b, tol=gtol, maxit=150, restart=5), refg, f"{shape} {sm} gmres(5)", slack=1)


# ---- c. initial guesses ---------------------------------------------------------------------------------------------------------
SOLVERS = [("pcg", None), ("pcg_sr", None), ("gmres", 7), ("gmres", 30)]


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
@pytest.mark.parametrize("device_vectors", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind,restart", SOLVERS, ids=["pcg", "pcg_sr", "gmres7", "gmres30"])
def test_initial_guess_matches_oracle_and_shift_identity(kind, restart, device_vectors, sm):
    """x holds the initial guess: history and solution of the oracle from the same x0, and on the device itself the history of
    (b, x0) equals that of (b - A x0, 0) with solution x0 + the other"""
    p, H, dev = _p25(sm)
    orc = _oracle(_case25, OSM[sm])
    A = H.levels[0].A.to_scipy().tocsr()
    b, x0 = rhs(p, 3), guess(p)
    tag = f"{kind}{restart or ''} {sm} {'device' if device_vectors else 'host'}"
    if kind == "gmres":
        kw = dict(tol=1e-9, maxit=150, restart=restart)
        ref = orc.gmres(b, x0=x0, tol=1e-9, maxit=150, restart=restart)
        cold = orc.gmres(b, tol=1e-9, maxit=1, restart=restart)[2][0]
    else:
        kw = dict(tol=1e-10, maxit=100)
        ref = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
        cold = orc.pcg(b, tol=1e-10, maxit=0)[2][0]
    assert abs(ref[2][0] - cold) > 0.1 * cold               # the guess moves err_0 far from the cold start's
    got = native_solve(dev, kind, b, x0, device_vectors=device_vectors, **kw)
    if kind == "gmres":
        _check_gmres(got, ref, tag)
    else:
        _check_pcg(got, ref, 1e-10, tag)
    f = p.free.astype(bool)
    assert np.linalg.norm((A @ got[0] - b)[f]) <= (1e-7 if kind == "gmres" else 1e-8) * np.linalg.norm(b)
    xs, its, es = native_solve(dev, kind, b - A @ x0, None, device_vectors=device_vectors, **kw)
    x, it, e = got
    if kind == "gmres":
        assert it == its and np.all(np.abs(e - es) <= 1e-6 * es[0]), tag
        assert rel(x, x0 + xs) <= 1e-7, tag
    else:
        k = min(it, its)
        assert abs(it - its) <= 1 and np.allclose(e[:k], es[:k], rtol=1e-6, atol=0), tag
        assert rel(x, x0 + xs) <= 1e-8, tag


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
@pytest.mark.parametrize("kind,restart", SOLVERS, ids=["pcg", "pcg_sr", "gmres7", "gmres30"])
def test_restart_from_the_solution_and_zero_rhs(kind, restart, sm):
    """x0 = the converged solution of a previous call: err_0 <= 1e-7 of the first call's and the residual stays converged;
    b = 0 from x0 != 0: the solver walks x to 0"""
    p, H, dev = _p25(sm)
    A = H.levels[0].A.to_scipy().tocsr()
    f = p.free.astype(bool)
    b = rhs(p, 3)
    kw = dict(restart=restart) if kind == "gmres" else {}
    for device_vectors in (True, False):
        x1, it1, e1 = native_solve(dev, kind, b, tol=1e-10, maxit=150, device_vectors=device_vectors, **kw)
        assert e1[-1] <= 1e-10 * e1[0]
        # three more iterations at most: the criterion 1e-10 * (the new, tiny err_0) is below the rounding level
        x2, it2, e2 = native_solve(dev, kind, b, x1, tol=1e-10, maxit=3, device_vectors=device_vectors, **kw)
        r1, r2 = np.linalg.norm((A @ x1 - b)[f]), np.linalg.norm((A @ x2 - b)[f])
        print(f"{kind}{restart or ''} {sm}: err_0 {e1[0]:.3e} -> {e2[0]:.3e}, residual {r1:.2e} -> {r2:.2e}")
        assert e2[0] <= 1e-7 * e1[0]
        assert np.all(np.isfinite(e2)) and r2 <= 1e-8 * np.linalg.norm(b) and rel(x2, x1) <= 1e-8
    x0 = guess(p)
    x, it, e = native_solve(dev, kind, np.zeros_like(b), x0, tol=1e-10, maxit=150, **kw)
    assert 0 < it < 150 and e[-1] <= 1e-10 * e[0]
    assert np.linalg.norm(x) <= 1e-8 * np.linalg.norm(x0)


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
@pytest.mark.parametrize("k", [4, 7])
def test_multi_pcg_initial_guesses_per_column(k, sm):
    """amgx_pcg_multi (fused groups 4 / 4 + 2 + 1 on the Jacobi handle, the column loop on the Gauss-Seidel one): a different guess
    per column, column 1 started at its own solution, column 2 with b = 0 and x0 = 0 -- each column against amgx_pcg with the
    same (b, x0) and against the oracle, both layouts, host and device vectors"""
    p, H, dev = _p25(sm)
    assert dev.multi_info(k)["fused"] == (1 if sm == "jacobi" else 0)
    orc = _oracle(_case25, OSM[sm])
    n = p.n
    B = np.stack([rhs(p, 20 + j) for j in range(k)])
    X0 = np.stack([guess(p, 40 + j) for j in range(k)])
    B[2] = 0.0
    X0[2] = 0.0
    sol1 = orc.pcg(B[1], tol=1e-12, maxit=100)[0]
    X0[1] = sol1
    cold1 = orc.pcg(B[1], tol=1e-10, maxit=0)[2][0]
    single = [native_solve(dev, "pcg", B[j], X0[j], tol=1e-10, maxit=40) for j in range(k)]
    refs = [orc.pcg(B[j], x0=X0[j], tol=1e-10, maxit=40) for j in range(k)]
    for interleaved in (False, True):
        for device_vectors in (True, False):
            X, its, errs = native_solve_multi(dev, B, X0, tol=1e-10, maxit=40, interleaved=interleaved, device_vectors=device_vectors)
            tag = f"k={k} {sm} il={int(interleaved)} dev={int(device_vectors)}"
            for j in range(k):
                if j == 2:                                   # nothing to do: bit-for-bit the zero guess
                    assert its[j] == 0 and errs[j].tolist() == [0.0] and not X[j].any() and not np.signbit(X[j]).any(), tag
                elif j == 1:                                 # started at the solution: the history is rounding noise, x stays
                    assert errs[j][0] <= 1e-7 * cold1 and rel(X[j], sol1) <= 1e-8, tag
                else:
                    _check_pcg((X[j], its[j], errs[j]), single[j], 1e-10, f"{tag} col {j} vs amgx_pcg")
                    _check_pcg((X[j], its[j], errs[j]), refs[j], 1e-10, f"{tag} col {j} vs oracle")


# ---- d. block systems -------------------------------------------------------------------------------------------------------------
# 6x6 with Jacobi is left out: the oracle's PCG does not converge within 100 iterations there (3x3 Jacobi 20, 3x3 gs_mc 14,
# 6x6 gs_mc 15 at 1e-10)
BLOCK_CASES = [("3x3", elasticity3, "jacobi"), ("3x3", elasticity3, "gs"), ("6x6", elasticity6, "gs")]


@functools.lru_cache(maxsize=None)
def _block_dev(name, sm, cycle="V"):
    case = elasticity3 if name == "3x3" else elasticity6
    p, H = case()
    return p, H, device_handle(H, sm_type=sm, mg_cycle=cycle)


@pytest.mark.parametrize("with_guess", [False, True], ids=["cold", "x0"])
@pytest.mark.parametrize("kind", ["pcg", "pcg_sr", "gmres12"])
@pytest.mark.parametrize("name,case,sm", BLOCK_CASES, ids=[f"{n}-{s}" for n, _, s in BLOCK_CASES])
def test_block_systems_match_oracle(name, case, sm, kind, with_guess):
    """3x3 and 6x6 elasticity: n counts scalar entries, the preconditioner runs the block kernels"""
    p, H, dev = _block_dev(name, sm)
    assert H.levels[0].A.br == (3 if name == "3x3" else 6) and dev.sizes[0] == p.n * p.bs
    orc = _oracle(case, OSM[sm])
    b = rhs(p, 3)
    x0 = guess(p) if with_guess else None
    tag = f"{name} {sm} {kind} {'x0' if with_guess else 'cold'}"
    for device_vectors in (True, False):
        if kind == "gmres12":
            ref = orc.gmres(b, x0=x0, tol=1e-9, maxit=150, restart=12)
            _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-9, maxit=150, restart=12, device_vectors=device_vectors), ref, tag)
        else:
            ref = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
            assert ref[1] < 100
            _check_pcg(native_solve(dev, kind, b, x0, tol=1e-10, maxit=100, device_vectors=device_vectors), ref, 1e-10, tag)


def test_block_system_w_cycle_and_multi_pcg():
    """a W-cycle handle on the 3x3 case, and amgx_pcg_multi (k = 3) there: block levels take the column loop"""
    p, H, dev = _block_dev("3x3", "gs", "W")
    orc = _oracle(elasticity3, "gs_mc", "W")
    b, x0 = rhs(p, 3), guess(p)
    _check_pcg(native_solve(dev, "pcg", b, x0, tol=1e-10, maxit=100), orc.pcg(b, x0=x0, tol=1e-10, maxit=100), 1e-10, "3x3 W pcg")
    _check_pcg(native_solve(dev, "pcg_sr", b, x0, tol=1e-10, maxit=100), orc.pcg(b, x0=x0, tol=1e-10, maxit=100), 1e-10, "3x3 W pcg_sr")
    _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-9, maxit=150, restart=12), orc.gmres(b, x0=x0, tol=1e-9, maxit=150, restart=12), "3x3 W gmres")
    for sm in ("jacobi", "gs"):
        p, H, dev = _block_dev("3x3", sm)
        mi = dev.multi_info(3)
        assert mi["fused"] == 0 and mi["groups"] == [1, 1, 1], mi
        orc = _oracle(elasticity3, OSM[sm])
        B = np.stack([rhs(p, 30 + j) for j in range(3)])
        X0 = np.stack([guess(p, 50), np.zeros(p.n * p.bs), guess(p, 52)])
        refs = [orc.pcg(B[j], x0=X0[j], tol=1e-10, maxit=100) for j in range(3)]
        for interleaved in (False, True):
            for device_vectors in (True, False):
                X, its, errs = native_solve_multi(dev, B, X0, tol=1e-10, maxit=100, interleaved=interleaved, device_vectors=device_vectors)
                for j in range(3):
                    _check_pcg((X[j], its[j], errs[j]), refs[j], 1e-10, f"3x3 {sm} multi il={int(interleaved)} col {j}")


# ---- e. documented argument edges ------------------------------------------------------------------------------------------------
def _raw(dev, fn, b, x, tol, maxit, pre, restart=None, flags=0, errs="yes", iters="yes"):
    """the C entry point itself on host vectors; errs / iters: 'yes' or None (NULL).  Returns (rc, iterations or None, errs or None)"""
    lib = dev._lib
    e = np.full(max(maxit, 0) + 1, -1.0) if errs else None
    it = C.c_int32(-7) if iters else None
    args = [dev._h, b.ctypes.data, x.ctypes.data, float(tol), int(maxit)] + ([] if restart is None else [int(restart)])
    rc = getattr(lib, fn)(*args, int(pre), int(flags), None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)),
                          None if it is None else C.byref(it))
    return rc, (None if it is None else int(it.value)), e


def test_maxit_zero_leaves_x_untouched():
    p, H, dev = _p25("jacobi")
    orc = _oracle(_case25, "jacobi")
    b, x0 = rhs(p, 3), guess(p)
    want = orc.pcg(b, x0=x0, tol=1e-10, maxit=0)[2][0]
    for kind in ("pcg", "pcg_sr"):
        for device_vectors in (True, False):
            x, it, errs = native_solve(dev, kind, b, x0, maxit=0, device_vectors=device_vectors)
            assert it == 0 and errs.shape == (1,) and np.array_equal(x, x0)
            assert abs(errs[0] - want) <= 1e-9 * want
    # amgx_gmres computes err_0 inside its first cycle: with maxit = 0 it does not touch errs (include/amgx.h), like the oracle
    x = x0.copy()
    rc, it, e = _raw(dev, "amgx_gmres", b, x, 1e-10, 0, 1, restart=5)
    assert rc == 0 and it == 0 and np.array_equal(x, x0) and e.tolist() == [-1.0]
    X, its, errs = native_solve_multi(dev, np.stack([b, 2 * b]), np.stack([x0, -x0]), maxit=0)
    assert its == [0, 0] and np.array_equal(X, np.stack([x0, -x0])) and abs(errs[0][0] - want) <= 1e-9 * want


def test_null_errs_and_iters_give_the_same_solution():
    """errs = NULL / iters = NULL (raw C call): bitwise the x of the call that passes both"""
    p, H, dev = _p25("gs")
    b, x0 = rhs(p, 3), guess(p)
    for fn, restart, flags in (("amgx_pcg", None, 0), ("amgx_pcg", None, 16), ("amgx_gmres", 7, 0)):
        xr = x0.copy()
        rc, it, e = _raw(dev, fn, b, xr, 1e-8, 60, 1, restart=restart, flags=flags)
        assert rc == 0 and 0 < it < 60 and e[it] <= 1e-8 * e[0] and np.all(e[it + 1:] == -1.0)      # nothing written past err_iters
        for errs, iters in ((None, "yes"), ("yes", None), (None, None)):
            x = x0.copy()
            rc, it2, e2 = _raw(dev, fn, b, x, 1e-8, 60, 1, restart=restart, flags=flags, errs=errs, iters=iters)
            assert rc == 0 and np.array_equal(x, xr), (fn, errs, iters)
            assert it2 in (None, it) and (e2 is None or np.array_equal(e2, e))
    # amgx_pcg_multi requires iters: an argument error, nothing runs
    B, X = np.stack([b, b]), np.stack([x0, x0])
    rc = dev._lib.amgx_pcg_multi(dev._h, 2, B.ctypes.data, p.n, X.ctypes.data, p.n, 1e-8, 10, 1, 0, None, None)
    assert rc != 0 and "iters == NULL" in dev._lib.amgx_last_error(dev._h).decode()
    assert np.array_equal(X, np.stack([x0, x0]))


def test_tolerance_above_one():
    """tol = 2: PCG tests after its first iteration (1 iteration), GMRES before it (0 iterations, x untouched)"""
    p, H, dev = _p25("jacobi")
    orc = _oracle(_case25, "jacobi")
    b = rhs(p, 3)
    xo, ito, eo = orc.pcg(b, tol=2.0, maxit=10)
    assert ito == 1
    for kind in ("pcg", "pcg_sr"):
        x, it, e = native_solve(dev, kind, b, tol=2.0, maxit=10)
        assert it == 1 and np.allclose(e, eo, rtol=1e-6, atol=0) and rel(x, xo) <= 1e-8
    xg, itg, eg = orc.gmres(b, tol=2.0, maxit=10, restart=7)
    x, it, e = native_solve(dev, "gmres", b, tol=2.0, maxit=10, restart=7)
    assert it == itg == 0 and not x.any() and np.allclose(e, eg, rtol=1e-9, atol=0) and e[0] > 0
    X, its, errs = native_solve_multi(dev, np.stack([b, -b]), tol=2.0, maxit=10)
    assert its == [1, 1] and rel(X[0], xo) <= 1e-8 and rel(X[1], -xo) <= 1e-8


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
def test_gmres_restart_lengths_and_partial_cycles(sm):
    p, H, dev = _p25(sm)
    orc = _oracle(_case25, OSM[sm])
    b, x0 = rhs(p, 3), guess(p)
    # stopped by maxit inside the second cycle: 10 iterations, and x carries the partial cycle's update
    ref = orc.gmres(b, x0=x0, tol=1e-30, maxit=10, restart=7)
    assert ref[1] == 10
    for device_vectors in (True, False):
        _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-30, maxit=10, restart=7, device_vectors=device_vectors), ref, f"{sm} gmres(7) maxit 10")
    x7 = orc.gmres(b, x0=x0, tol=1e-30, maxit=7, restart=7)[0]
    assert rel(ref[0], x7) > 1e-5                            # (the check above would see a missing update)
    # restart = 1 (minimal residual steps), 40 (the largest allowed), 45 > maxit = 20
    ref = orc.gmres(b, x0=x0, tol=1e-6, maxit=60, restart=1)
    _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-6, maxit=60, restart=1), ref, f"{sm} gmres(1)")
    assert np.all(np.diff(ref[2]) <= 1e-12 * ref[2][0])
    ref = orc.gmres(b, x0=x0, tol=1e-9, maxit=150, restart=40)
    _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-9, maxit=150, restart=40), ref, f"{sm} gmres(40)")
    # (restart > maxit: the oracle takes the length as it comes; the device solver is held to 40)
    ref = orc.gmres(b, x0=x0, tol=1e-30, maxit=20, restart=40)
    assert ref[1] == 20
    _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-30, maxit=20, restart=40), ref, f"{sm} gmres(40) maxit 20")
    ref = orc.gmres(b, tol=1e-30, maxit=5, restart=30)
    _check_gmres(native_solve(dev, "gmres", b, tol=1e-30, maxit=5, restart=30), ref, f"{sm} gmres(30) maxit 5")


def test_argument_errors_return_before_any_work():
    """restart = 41 (documented limit), restart = 0, maxit = -1: non-zero return, the message, x untouched"""
    from ngsamg_amd._lib import NgsAMGError
    p, H, dev = _p25("jacobi")
    b, x0 = rhs(p, 3), guess(p)
    x = x0.copy()
    rc, it, e = _raw(dev, "amgx_gmres", b, x, 1e-8, 20, 1, restart=41)
    assert rc != 0 and "restart lengths above 40 are not supported (got 41)" in dev._lib.amgx_last_error(dev._h).decode()
    assert np.array_equal(x, x0) and it == -7 and np.all(e == -1.0)
    rc, it, e = _raw(dev, "amgx_gmres", b, x, 1e-8, 20, 1, restart=45)
    assert rc != 0 and "(got 45)" in dev._lib.amgx_last_error(dev._h).decode()
    rc, it, e = _raw(dev, "amgx_gmres", b, x, 1e-8, 20, 1, restart=0)
    assert rc != 0 and "amgx_gmres: bad arguments" in dev._lib.amgx_last_error(dev._h).decode()
    rc, it, e = _raw(dev, "amgx_gmres", b, x, 1e-8, -1, 1, restart=5)
    assert rc != 0 and "amgx_gmres: bad arguments" in dev._lib.amgx_last_error(dev._h).decode()
    rc, it, e = _raw(dev, "amgx_pcg", b, x, 1e-8, -1, 1)
    assert rc != 0 and "amgx_pcg: bad arguments" in dev._lib.amgx_last_error(dev._h).decode()
    its = np.zeros(2, dtype=np.int32)
    B, X = np.stack([b, b]), np.stack([x0, x0])
    rc = dev._lib.amgx_pcg_multi(dev._h, 2, B.ctypes.data, p.n, X.ctypes.data, p.n, 1e-8, -1, 1, 0, None, its.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc != 0 and "maxit < 0" in dev._lib.amgx_last_error(dev._h).decode()
    assert np.array_equal(x, x0) and np.array_equal(X, np.stack([x0, x0]))
    with pytest.raises(NgsAMGError, match="restart lengths above 40"):
        native_solve(dev, "gmres", b, x0, restart=41)
    # the handle works as before
    ref = _oracle(_case25, "jacobi").pcg(b, x0=x0, tol=1e-10, maxit=100)
    _check_pcg(native_solve(dev, "pcg", b, x0, tol=1e-10, maxit=100), ref, 1e-10, "after the errors")


def test_gmres_without_preconditioner_and_solvers_on_host_vectors():
    p, H, dev = _p25("gs")
    orc = _oracle(_case25, "gs_mc")
    b, x0 = rhs(p, 3), guess(p)
    ref = orc.gmres(b, x0=x0, tol=1e-30, maxit=25, restart=10, precond=False)
    for device_vectors in (True, False):
        _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-30, maxit=25, restart=10, pre=False, device_vectors=device_vectors), ref,
                     f"gmres(10) without preconditioner dev={int(device_vectors)}")
    refp, refg = orc.pcg(b, tol=1e-10, maxit=100), orc.gmres(b, tol=1e-9, maxit=150, restart=12)
    _check_pcg(native_solve(dev, "pcg_sr", b, tol=1e-10, maxit=100, device_vectors=False), refp, 1e-10, "pcg_sr host")
    _check_gmres(native_solve(dev, "gmres", b, tol=1e-9, maxit=150, restart=12, device_vectors=False), refg, "gmres(12) host")


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
def test_single_reduction_flag_without_preconditioner_is_the_classical_call(sm):
    """AMGX_PCG_SINGLE_REDUCTION with use_precond = 0 falls back to the classical form: bitwise the same x and history"""
    p, H, dev = _p25(sm)
    b, x0 = rhs(p, 3), guess(p)
    for device_vectors in (True, False):
        a = native_solve(dev, "pcg", b, x0, tol=1e-30, maxit=15, pre=False, device_vectors=device_vectors)
        c = native_solve(dev, "pcg_sr", b, x0, tol=1e-30, maxit=15, pre=False, device_vectors=device_vectors)
        assert a[1] == c[1] == 15 and np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2])
    ref = _oracle(_case25, OSM[sm]).pcg(b, x0=x0, tol=1e-30, maxit=15, precond=False)
    assert np.allclose(a[2], ref[2], rtol=1e-8, atol=0)


def test_solvers_on_a_colour_major_handle():
    """AMGX_GS_PERM=1 at create time: the Gauss-Seidel levels, level 0 included, are stored in colour-major numbering and the solvers
    work on staged, renumbered copies of b and x -- unchanged for the caller"""
    for case, tagc in ((_case17, "poisson17"), (elasticity3, "3x3")):
        p, H = case()
        dev = device_handle(H, {"AMGX_GS_PERM": "1"}, sm_type="gs")
        orc = _oracle(case, "gs_mc")
        b, x0 = rhs(p, 3), guess(p)
        refp = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
        refg = orc.gmres(b, x0=x0, tol=1e-9, maxit=150, restart=12)
        for device_vectors in (True, False):
            tag = f"GS_PERM {tagc} dev={int(device_vectors)}"
            _check_pcg(native_solve(dev, "pcg", b, x0, tol=1e-10, maxit=100, device_vectors=device_vectors), refp, 1e-10, tag + " pcg")
            _check_pcg(native_solve(dev, "pcg_sr", b, x0, tol=1e-10, maxit=100, device_vectors=device_vectors), refp, 1e-10, tag + " pcg_sr")
            _check_gmres(native_solve(dev, "gmres", b, x0, tol=1e-9, maxit=150, restart=12, device_vectors=device_vectors), refg, tag + " gmres")
            B = np.stack([b, rhs(p, 4)])
            X0 = np.stack([x0, guess(p, 6)])
            refs = [refp, orc.pcg(B[1], x0=X0[1], tol=1e-10, maxit=100)]
            for interleaved in (False, True):
                X, its, errs = native_solve_multi(dev, B, X0, tol=1e-10, maxit=100, interleaved=interleaved, device_vectors=device_vectors)
                for j in range(2):
                    _check_pcg((X[j], its[j], errs[j]), refs[j], 1e-10, f"{tag} multi il={int(interleaved)} col {j}")


# ---- f. handle state ---------------------------------------------------------------------------------------------------------------
def _sequence(p):
    b, x0 = rhs(p, 3), guess(p)
    B = np.stack([rhs(p, 60 + j) for j in range(4)])
    X0 = np.stack([guess(p, 70 + j) for j in range(4)])
    return [("gmres30", lambda d: native_solve(d, "gmres", b, x0, tol=1e-9, maxit=150, restart=30)),
            ("pcg", lambda d: native_solve(d, "pcg", b, x0, tol=1e-10, maxit=100)),
            ("pcg_sr", lambda d: native_solve(d, "pcg_sr", b, x0, tol=1e-10, maxit=100)),
            ("gmres5", lambda d: native_solve(d, "gmres", b, x0, tol=1e-9, maxit=150, restart=5)),
            ("gmres40", lambda d: native_solve(d, "gmres", b, x0, tol=1e-9, maxit=150, restart=40)),       # the basis buffer grows
            ("multi4", lambda d: native_solve_multi(d, B, X0, tol=1e-10, maxit=100)),
            ("mult", lambda d: _mult(d, b)),
            ("pcg again", lambda d: native_solve(d, "pcg", b, x0, tol=1e-10, maxit=100))]


def _mult(dev, b):
    import torch
    xd = torch.full((b.size,), float("nan"), dtype=torch.float64, device="cuda")
    dev.Mult(torch.from_numpy(b).cuda(), xd)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), 0, np.zeros(1)


def _same(a, c):
    """bitwise: x (or the k solutions), iteration counts, the whole history"""
    if not np.array_equal(np.asarray(a[0]), np.asarray(c[0])) or a[1] != c[1]:
        return False
    ea, ec = (a[2], c[2]) if isinstance(a[2], list) else ([a[2]], [c[2]])
    return len(ea) == len(ec) and all(np.array_equal(u, v) for u, v in zip(ea, ec))


@pytest.mark.parametrize("sm", ["jacobi", "gs"])
def test_solvers_sharing_one_handle_do_not_disturb_each_other(sm):
    """the solvers keep their work vectors in the handle (grow-only, shared between PCG, single-reduction PCG and GMRES; the cycle's
    graphs are keyed on their addresses): a sequence of different solvers on ONE handle gives, call by call, bitwise the result of
    the same call on a fresh handle; a handle without graphs gives bitwise the results of one with graphs"""
    p, H = _case25()
    shared = device_handle(H, sm_type=sm)
    direct = device_handle(H, sm_type=sm, use_graph=False)
    seq = _sequence(p)
    got = {}
    for name, call in seq:
        got[name] = call(shared)
        fresh = call(device_handle(H, sm_type=sm))
        assert _same(got[name], fresh), f"{sm}: {name} on the shared handle differs from a fresh handle"
        assert _same(got[name], call(direct)), f"{sm}: {name} without graphs differs from the run with graphs"
    assert _same(got["pcg"], got["pcg again"])
    assert got["pcg"][1] > 5 and got["gmres40"][1] > 5
