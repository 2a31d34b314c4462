"""The references of the Krylov solver tests, pinned on the CPU: the oracle's pcg / gmres with an initial guess against a plain
numpy statement of the recurrence, the edge semantics the device solvers are held to (tests/test_gpu_krylov_edges.py), and the torch
CGSolver (check_every, sol=) on CPU tensors."""
import numpy as np
import pytest

from tests.krylov_cases import elasticity3, elasticity6, free_mask, guess, numpy_pcg, rel
from tests.problems import poisson_case, rhs


def _poisson17():
    return poisson_case((17, 17, 17), "right|top", 20)


def _poisson25():
    return poisson_case((25, 25, 25), "right|top", 20)


# 6x6 elasticity with Jacobi is left out of the converged runs: the oracle's PCG does not reach 1e-10 within 100 iterations there
SYSTEMS = [("poisson17", _poisson17, "jacobi"), ("poisson17", _poisson17, "gs_mc"), ("elast3", elasticity3, "jacobi"),
           ("elast3", elasticity3, "gs_mc"), ("elast6", elasticity6, "gs_mc")]
SHIFT_SYSTEMS = [("poisson25", _poisson25, "jacobi"), ("poisson25", _poisson25, "gs_mc")] + SYSTEMS[2:]
IDS = [f"{n}-{s}" for n, _, s in SYSTEMS]
SHIFT_IDS = [f"{n}-{s}" for n, _, s in SHIFT_SYSTEMS]


@pytest.mark.parametrize("name,case,osm", SYSTEMS, ids=IDS)
def test_oracle_pcg_with_initial_guess_equals_numpy_pcg(name, case, osm):
    """Oracle.pcg(b, x0) against the textbook recurrence in numpy (scipy level-0 matrix, Oracle.apply as the preconditioner): same
    count, whole history to 1e-9, solution to 1e-8"""
    from oracle.pyoracle import Oracle
    p, H = case()
    orc = Oracle(H.levels, sm_type=osm)
    A = H.levels[0].A.to_scipy().tocsr()
    b, x0 = rhs(p, 3), guess(p)
    x0_in = x0.copy()
    xo, ito, eo = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
    assert np.array_equal(x0, x0_in)                         # the caller's guess is copied, not overwritten
    xn, itn, en = numpy_pcg(A, lambda v: orc.apply(v.copy()), b, x0, 1e-10, 100)
    cold = orc.pcg(b, tol=1e-10, maxit=100)[2][0]
    print(f"{name} {osm}: it {ito} / {itn}, history {np.max(np.abs(eo - en[:eo.size]) / en[:eo.size]):.1e}, solution {rel(xo, xn):.1e}, "
          f"err_0 warm / cold {eo[0] / cold:.1f}")
    assert ito == itn and ito < 100
    assert eo.shape == en.shape and np.allclose(eo, en, rtol=1e-9, atol=0)
    assert rel(xo, xn) <= 1e-8
    assert abs(eo[0] - cold) > 0.01 * cold                   # the guess matters: a solver that ignored it would be seen


@pytest.mark.parametrize("name,case,osm", SHIFT_SYSTEMS, ids=SHIFT_IDS)
def test_oracle_shift_identity(name, case, osm):
    """pcg(b, x0) has the history of pcg(b - A x0, 0) and the solution x0 + that one's; the same for GMRES(7)"""
    from oracle.pyoracle import Oracle
    p, H = case()
    orc = Oracle(H.levels, sm_type=osm)
    A = H.levels[0].A.to_scipy().tocsr()
    b, x0 = rhs(p, 3), guess(p)
    x, it, e = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
    xs, its, es = orc.pcg(b - A @ x0, tol=1e-10, maxit=100)
    assert it == its and np.allclose(e, es, rtol=1e-9, atol=0)
    assert rel(x, x0 + xs) <= 1e-8
    x, it, e = orc.gmres(b, x0=x0, tol=1e-9, maxit=45, restart=7)
    xs, its, es = orc.gmres(b - A @ x0, tol=1e-9, maxit=45, restart=7)
    assert it == its and np.all(np.abs(e - es) <= 1e-9 * es[0])
    assert rel(x, x0 + xs) <= 1e-8


def test_oracle_gmres_with_initial_guess_minimises_the_preconditioned_residual():
    """test_oracle_gmres_minimises_the_preconditioned_residual from a non-zero x0: the recurrence value is the true |C (b - A x)|,
    monotone inside a cycle, and the solution is PCG's from the same guess"""
    from oracle.pyoracle import Oracle
    p, H = poisson_case((13, 13, 13), "right|top", 20)
    orc = Oracle(H.levels, sm_type="jacobi")
    A = H.levels[0].A.to_scipy()
    b, x0 = rhs(p, 3), guess(p)
    x, it, errs = orc.gmres(b, x0=x0, tol=1e-10, maxit=100, restart=40)
    xc, itc, _ = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
    assert errs[-1] <= 1e-10 * errs[0] and it <= itc + 1
    assert abs(errs[0] - np.linalg.norm(orc.apply(b - A @ x0))) <= 1e-12 * errs[0]
    assert all(e2 <= e1 * (1 + 1e-12) for e1, e2 in zip(errs[:-1], errs[1:]))
    assert abs(np.linalg.norm(orc.apply(b - A @ x)) - errs[-1]) <= 1e-6 * errs[0]
    assert np.linalg.norm(x - xc) <= 1e-7 * np.linalg.norm(xc)
    for restart in (5, 7):                                   # restarted: monotone inside every cycle, same fixed point
        xr, itr, er = orc.gmres(b, x0=x0, tol=1e-10, maxit=300, restart=restart)
        assert itr >= it and np.linalg.norm(xr - xc) <= 1e-7 * np.linalg.norm(xc)
        for c0 in range(0, itr, restart):
            cyc = er[c0:c0 + restart + 1]
            assert all(e2 <= e1 * (1 + 1e-12) for e1, e2 in zip(cyc[:-1], cyc[1:]))
        assert abs(np.linalg.norm(orc.apply(b - A @ xr)) - er[-1]) <= 1e-6 * er[0]


@pytest.mark.parametrize("name,case,osm", [SYSTEMS[0], SYSTEMS[2], SYSTEMS[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_oracle_edge_semantics(name, case, osm):
    """facts the device tests inherit: what maxit = 0, b = 0, tol >= 1 and a stop inside a restart cycle give"""
    from oracle.pyoracle import Oracle
    p, H = case()
    orc = Oracle(H.levels, sm_type=osm)
    A = H.levels[0].A.to_scipy()
    b, x0 = rhs(p, 3), guess(p)
    # maxit = 0: err_0 is computed, x is untouched
    x, it, e = orc.pcg(b, x0=x0, tol=1e-10, maxit=0)
    r0 = b - A @ x0
    assert it == 0 and e.shape == (1,) and np.array_equal(x, x0)
    assert abs(e[0] - np.sqrt(abs(orc.apply(r0) @ r0))) <= 1e-12 * e[0]
    # GMRES computes err_0 inside its first cycle: with maxit = 0 nothing runs and errs[0] is left as the caller passed it (0 here)
    x, it, e = orc.gmres(b, x0=x0, tol=1e-10, maxit=0, restart=5)
    assert it == 0 and np.array_equal(x, x0) and e.tolist() == [0.0]
    # b = 0 from x = 0: nothing to do
    for x, it, e in (orc.pcg(0 * b, tol=1e-10, maxit=10), orc.gmres(0 * b, tol=1e-10, maxit=10, restart=5)):
        assert it == 0 and e.tolist() == [0.0] and not x.any()
    # b = 0 from a guess: converges to 0
    x, it, e = orc.pcg(0 * b, x0=x0, tol=1e-10, maxit=100)
    assert 0 < it < 100 and np.linalg.norm(x) <= 1e-8 * np.linalg.norm(x0)
    # tol >= 1: PCG tests after its first iteration, GMRES before it
    x, it, e = orc.pcg(b, tol=2.0, maxit=10)
    assert it == 1 and e.shape == (2,) and x.any()
    x, it, e = orc.gmres(b, tol=2.0, maxit=10, restart=7)
    assert it == 0 and e.shape == (1,) and e[0] > 0 and not x.any()
    # GMRES(7) stopped by maxit = 10 inside its second cycle: the partial cycle's update is applied
    x, it, e = orc.gmres(b, tol=1e-30, maxit=10, restart=7)
    assert it == 10 and e.shape == (11,)
    assert abs(np.linalg.norm(orc.apply(b - A @ x)) - e[-1]) <= 1e-6 * e[0]
    x7 = orc.gmres(b, tol=1e-30, maxit=7, restart=7)[0]
    assert abs(np.linalg.norm(orc.apply(b - A @ x7)) - e[7]) <= 1e-6 * e[0] and e[-1] < e[7]


# ---- the torch CGSolver on CPU tensors ---------------------------------------------------------------------------------------
class _Mat:
    def __init__(self, A):
        self.A = A

    def MatVec(self, level, x, y):
        import torch
        assert level == 0
        y.copy_(torch.from_numpy(self.A @ x.numpy()))


class _Pre:
    def __init__(self, orc):
        self.orc = orc

    def Mult(self, b, x):
        import torch
        x.copy_(torch.from_numpy(self.orc.apply(b.numpy().copy())))


@pytest.mark.parametrize("name,case,osm", [SYSTEMS[0], SYSTEMS[3]], ids=[IDS[0], IDS[3]])
def test_torch_cgsolver_check_every_and_initial_guess(name, case, osm):
    """CGSolver(check_every = m) only moves the host look-ups: iterations, errors (bitwise) and the callback sequence up to the
    stopping index are those of check_every = 1; sol = x0 reproduces the oracle's pcg(b, x0)"""
    import torch
    from ngsamg_amd.krylov import CGSolver
    from oracle.pyoracle import Oracle
    p, H = case()
    orc = Oracle(H.levels, sm_type=osm)
    A = H.levels[0].A.to_scipy().tocsr()
    b, x0 = rhs(p, 3), guess(p)
    xo, ito, eo = orc.pcg(b, x0=x0, tol=1e-10, maxit=100)
    ref = None
    for ce in (1, 2, 3, 7, 1000):
        cb = []
        cg = CGSolver(_Mat(A), _Pre(orc), tol=1e-10, maxsteps=100, callback=lambda k, e: cb.append((k, e)), check_every=ce)
        sol = torch.from_numpy(x0.copy())
        x = cg.Solve(torch.from_numpy(b), sol)
        assert x is sol                                      # the guess is updated in place and returned
        if ref is None:
            ref = (cg.iterations, list(cg.errors), list(cb))
            assert cg.iterations == ito and len(cb) == ito and [k for k, _ in cb] == list(range(1, ito + 1))
            assert np.allclose(cg.errors, eo, rtol=1e-9, atol=0)
        assert cg.iterations == ref[0] and cg.errors == ref[1], ce
        assert cb[:cg.iterations] == ref[2], ce
        assert len(cb) == min(100, -(-cg.iterations // ce) * ce), ce       # surplus iterations up to the next look-up
        assert [e for _, e in cb[:cg.iterations]] == cg.errors[1:]
        assert rel(x.numpy(), xo) <= 1e-8, ce
    # cold start: sol = None allocates the zero guess
    cg = CGSolver(_Mat(A), _Pre(orc), tol=1e-10, maxsteps=100)
    x = cg.Solve(torch.from_numpy(b))
    xc, itc, ec = orc.pcg(b, tol=1e-10, maxit=100)
    assert cg.iterations == itc and np.allclose(cg.errors, ec, rtol=1e-9, atol=0) and rel(x.numpy(), xc) <= 1e-8
    # without a preconditioner
    cg = CGSolver(_Mat(A), None, tol=1e-30, maxsteps=12)
    cg.Solve(torch.from_numpy(b), torch.from_numpy(x0.copy()))
    _, itp, ep = orc.pcg(b, x0=x0, tol=1e-30, maxit=12, precond=False)
    assert cg.iterations == itp == 12 and np.allclose(cg.errors, ep, rtol=1e-9, atol=0)


def test_torch_cgsolver_zero_residual_returns_at_once():
    import torch
    from ngsamg_amd.krylov import CGSolver
    from oracle.pyoracle import Oracle
    p, H = _poisson17()
    orc = Oracle(H.levels, sm_type="jacobi")
    A = H.levels[0].A.to_scipy().tocsr()
    calls = []
    cg = CGSolver(_Mat(A), _Pre(orc), tol=1e-10, maxsteps=50, callback=lambda k, e: calls.append(k), check_every=3)
    x = cg.Solve(torch.zeros(p.n, dtype=torch.float64))
    assert cg.iterations == 0 and cg.errors == [0.0] and not calls and not x.any()
    # maxsteps reached without convergence: the full history, iterations = maxsteps
    b = rhs(p, 3)
    cg = CGSolver(_Mat(A), _Pre(orc), tol=1e-30, maxsteps=7, check_every=3)
    cg.Solve(torch.from_numpy(b))
    _, it, e = orc.pcg(b, tol=1e-30, maxit=7)
    assert cg.iterations == it == 7 and np.allclose(cg.errors, e, rtol=1e-9, atol=0)
    assert np.count_nonzero(free_mask(p)) < p.n
