"""Chebyshev polynomial smoother: the numpy reference of tests/cheby_ref.py against the oracle, and the descriptor (no GPU).

Tolerances: the reference restates the oracle's Jacobi cycle with another summation order only -> 1e-13; PCG
iteration budgets come from the oracle's own sequential Gauss-Seidel count on the same problem and right-hand side."""
import ctypes as C

import numpy as np
import pytest

from tests.cheby_ref import ChebyRef, LevelOps, cheby_coefficients, lambda_true, power_estimate
from tests.problems import elasticity_case, poisson_case, rhs


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _cases():
    return [("poisson2d", poisson_case((33, 33), "left|top", 5)), ("poisson3d", poisson_case((17, 17, 17), "right|top", 20)),
            ("elast3x3", elasticity_case((9, 7, 7), False, 10)), ("elast6x6", elasticity_case((9, 7, 7), True, 10))]


def _lmax(H, steps=20):
    """explicit per-level interval ends: 1.1 x a 20-step power-iteration estimate (any start vector: here the device's)"""
    return [1.1 * power_estimate(lv, steps) for lv in H.levels[:-1]] + [1.0]


# ---- 1. the reference with Jacobi is the oracle's Jacobi cycle ------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
def test_reference_with_jacobi_equals_oracle(cycle):
    from oracle.pyoracle import Oracle
    for name, (p, H) in _cases():
        b = rhs(p, 2)
        ref = Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b)
        got = ChebyRef(H, sm="jacobi", cycle=cycle).apply(b)
        e = _rel(got, ref)
        print(name, cycle, e)
        assert e < 1e-13, (name, cycle, e)


def test_reference_flag_contract_with_jacobi_equals_oracle():
    from oracle.pyoracle import Oracle
    p, H = poisson_case((33, 33), "left|top", 5)
    A = H.levels[0].A.to_scipy()
    rng = np.random.default_rng(5)
    for steps, symm in ((1, False), (2, False), (1, True), (2, True)):
        orc = Oracle(H.levels, sm_type="jacobi", sm_steps=steps, sm_symm=symm)
        ref = ChebyRef(H, sm="jacobi", sm_steps=steps, sm_symm=symm)
        for back in (False, True):
            for ru in (False, True):
                for ur in (False, True):
                    for xz in (False, True):
                        b = rhs(p, 7)
                        x = np.zeros(p.n) if xz else rng.standard_normal(p.n) * p.free
                        res = (b - A @ x) if ru else rng.standard_normal(p.n)
                        xo, ro = x.copy(), res.copy()
                        orc.smooth(0, xo, b, ro, ru, ur, xz, back)
                        xr, rr = x.copy(), res.copy()
                        ref.smooth(0, xr, b, rr, ru, ur, xz, back)
                        assert _rel(xr, xo) < 1e-13, (steps, symm, back, ru, ur, xz)
                        if ur:
                            assert _rel(rr, ro) < 1e-12, (steps, symm, back, ru, ur, xz)


# ---- 2. degree 1 is Jacobi with omega = 1 / theta -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W"])
def test_degree_one_is_jacobi_with_omega_one_over_theta(cycle):
    from oracle.pyoracle import Oracle
    lmax, ratio = 2.2, 10.0
    theta = 0.5 * (lmax + lmax / ratio)
    assert cheby_coefficients(lmax, ratio, 1)[0] == 1.0 / theta
    for name, (p, H) in _cases():
        b = rhs(p, 4)
        ref = Oracle(H.levels, sm_type="jacobi", omega=1.0 / theta, cycle=cycle).apply(b)
        got = ChebyRef(H, sm="cheby", degree=1, ratio=ratio, lambda_max=[lmax] * H.n_levels, cycle=cycle).apply(b)
        e = _rel(got, ref)
        print(name, cycle, e)
        assert e < 1e-13, (name, cycle, e)


def test_coefficients_are_the_chebyshev_recurrence():
    """x_k - x* = p_k(Dinv A)(x_0 - x*) with p_k(t) = T_k((theta - t)/delta) / T_k(sigma): checked on a diagonal operator"""
    lmax, ratio, k = 2.0, 10.0, 5
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    c0, c1, c2 = cheby_coefficients(lmax, ratio, k)
    t = np.linspace(0.05, 2.0, 41)            # eigenvalues; b = 0, so the iterate is the error
    x = np.ones_like(t)
    d = c0 * (0.0 - t * x)
    x = x + d
    for j in range(2, k + 1):
        d = c1[j] * d + c2[j] * (0.0 - t * x)
        x = x + d
    T = np.polynomial.chebyshev.Chebyshev.basis(k)
    assert np.allclose(x, T((theta - t) / delta) / T(theta / delta), rtol=0, atol=1e-13)


# ---- 3. the preconditioner is symmetric -----------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_reference_preconditioner_is_symmetric(degree):
    for name, (p, H) in _cases():
        ref = ChebyRef(H, sm="cheby", degree=degree, lambda_max=_lmax(H))
        u, v = rhs(p, 11), rhs(p, 12)
        a, b = float(u @ ref.apply(v)), float(v @ ref.apply(u))
        print(name, degree, abs(a - b) / abs(a))
        assert abs(a - b) <= 1e-12 * abs(a), (name, degree, a, b)


# ---- 4. iteration budgets -------------------------------------------------------------------------------------------------
def _table_cases():
    p1, H1 = poisson_case((24, 24, 24), "right|top", 20)
    p2, H2 = elasticity_case((10, 10, 10), False, 20)
    p3, H3 = elasticity_case((10, 10, 10), True, 20)
    return [("poisson 24^3", p1, H1, rhs(p1, 0)), ("elasticity 10^3 displacements", p2, H2, p2.load),
            ("elasticity 10^3 rotations", p3, H3, p3.load)]


def test_pcg_iteration_budgets():
    """PCG to 1e-8, V(1,1): degree 2 needs no more iterations than the oracle's sequential Gauss-Seidel on the three problems of
    the design table; degree 1 repairs block Jacobi on the rotational problem (<= 20 where omega = 0.9 needs > 100)."""
    from oracle.pyoracle import Oracle
    for name, p, H, b in _table_cases():
        b = np.ascontiguousarray(b, dtype=np.float64)
        lm = _lmax(H)
        _, it_gs, _ = Oracle(H.levels, sm_type="gs").pcg(b, tol=1e-8, maxit=300)
        _, it_jac, _ = Oracle(H.levels, sm_type="jacobi").pcg(b, tol=1e-8, maxit=300)
        its = {k: ChebyRef(H, sm="cheby", degree=k, lambda_max=lm).pcg(b, tol=1e-8, maxit=300)[1] for k in (1, 2, 3)}
        print(f"{name}: levels {[lv.n for lv in H.levels]} jacobi {it_jac} gs {it_gs} cheby {its} lmax {[round(v, 3) for v in lm]}")
        assert its[2] <= it_gs, (name, its, it_gs)
        assert its[3] <= its[2] <= its[1], (name, its)
        if "rotations" in name:
            assert it_jac > 100, (name, it_jac)
            assert its[1] <= 20, (name, its)


def test_power_estimate_brackets_lambda_max():
    """what the device's estimator promises, on the CPU restatement: 30 steps from the device's start vector give a lower bound
    within 10 % of lambda_max(Dinv A), so 1.1 x estimate lies in [lambda_max, 1.1 lambda_max]"""
    for name, (p, H) in _cases():
        for l, lv in enumerate(H.levels[:-1]):
            est, true = power_estimate(lv, 30), lambda_true(lv)
            print(name, l, lv.n, est, true, est / true)
            assert true <= 1.1 * est <= 1.1 * true * (1 + 1e-10), (name, l, est, true)


# ---- 5. the descriptor ----------------------------------------------------------------------------------------------------
def test_descriptor_carries_the_chebyshev_fields():
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = poisson_case((33, 33), "left|top", 5)
    desc, keep, _ = hierarchy_desc(H, sm_type="cheby", cheb_degree=3)
    assert _lib.AMGX_SM_CHEBY == 3
    for i in range(H.n_levels):
        d = desc.levels[i]
        assert (d.sm_type, d.cheb_degree, d.cheb_lambda_max, d.cheb_ratio) == (3, 3, 0.0, 0.0)
    n = H.n_levels
    lam = [2.0 + i for i in range(n)]
    desc, keep, _ = hierarchy_desc(H, sm_type=["cheby"] + ["gs"] * (n - 1), cheb_degree=list(range(1, n + 1)), cheb_ratio=4.0, cheb_lambda_max=lam)
    assert (desc.levels[0].sm_type, desc.levels[0].cheb_degree, desc.levels[0].cheb_lambda_max, desc.levels[0].cheb_ratio) == (3, 1, 2.0, 4.0)
    assert (desc.levels[1].sm_type, desc.levels[1].cheb_degree, desc.levels[1].cheb_lambda_max, desc.levels[1].cheb_ratio) == (1, 0, 0.0, 0.0)
    # zero-initialised descriptors mean defaults
    z = _lib.amgx_level_desc()
    assert (z.cheb_degree, z.cheb_lambda_max, z.cheb_ratio) == (0, 0.0, 0.0)
    for bad in (dict(cheb_degree=0), dict(cheb_degree=9), dict(cheb_degree=-1), dict(cheb_ratio=1.0), dict(cheb_ratio=0.5),
                dict(cheb_ratio=-3), dict(cheb_lambda_max=-1.0), dict(cheb_degree=[2])):
        with pytest.raises(_lib.NgsAMGError):
            hierarchy_desc(H, sm_type="cheby", **bad)
    with pytest.raises(_lib.NgsAMGError, match="cheby"):
        hierarchy_desc(H, sm_type="chebyshev")
    assert "amgx_smoother_info" in _lib.AMGX_SYMBOLS
    assert C.sizeof(_lib.amgx_level_desc) % 8 == 0


def test_preconditioner_flags_select_the_type():
    """ngs_amg_sm_type = "cheby" (also per level) reaches the descriptor; every other unknown string still falls back to gs"""
    import ngsamg_amd.NgsAMG as N
    seen = {}

    class Probe:
        def __init__(self, hier, **kw):
            seen.update(kw)
            raise N.NgsAMGError("probe")

    p, H = poisson_case((17, 17), "left|top", 5)
    old = N.DeviceAMGMatrix
    N.DeviceAMGMatrix = Probe
    try:
        from tests.problems import to_matrix
        for flags, want in ((dict(ngs_amg_sm_type="cheby", ngs_amg_cheb_degree=3, ngs_amg_cheb_ratio=20), "cheby"),
                            (dict(ngs_amg_sm_type="dyn_block_gs"), "hgs"),
                            (dict(ngs_amg_sm_type="jacobi", ngs_amg_sm_type_spec=["cheby"]), "cheby")):
            with pytest.raises(N.NgsAMGError, match="probe"):
                N.h1_scal(to_matrix(p), p.free, p.coords, ngs_amg_dim=2, ngs_amg_max_coarse_size=5, **flags)
            assert seen["sm_type"][0] == want, (flags, seen["sm_type"])
            if "ngs_amg_cheb_degree" in flags:
                assert seen["cheb_degree"] == 3 and seen["cheb_ratio"] == 20.0
            else:
                assert seen["cheb_degree"] == 2 and seen["cheb_ratio"] == 10.0
    finally:
        N.DeviceAMGMatrix = old
