"""ngsamg_amd.eigen.lobpcg on the numpy backend: PINVIT and LOBPCG, with and without a lumped mass matrix, preconditioned by
the oracle's V(1,1) cycle (Poisson) and by the Chebyshev cycle of tests/cheby_ref.py (elasticity); the safeguards.

Bounds (tests/eigen_cases.py): |theta_j - lambda_j| <= res_j |theta_j| kappa (Krylov-Weinstein, kappa = |M^-1/2|, 1 without mass)
plus the reference's own bound; |X^T M X - I|_max <= 1e-10."""
import numpy as np
import pytest

from ngsamg_amd._lib import NgsAMGError
from ngsamg_amd.eigen import lobpcg
from ngsamg_amd.multivector import HostMultiVector
from tests import eigen_cases as ec

KIND = {"poisson": "jacobi", "elast": "cheby"}


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("name", ["poisson", "elast"])
def test_reference_spectrum_has_a_gap(name, with_mass):
    ec.assert_gap(name, with_mass)


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("history", [False, True], ids=["pinvit", "lobpcg"])
@pytest.mark.parametrize("name", ["poisson", "elast"])
def test_eigenpairs(name, history, with_mass):
    ec.assert_gap(name, with_mass)
    lams, X, info, seen = ec.host_run(name, KIND[name], history, with_mass)
    ec.check_result(name, lams, X, info, with_mass, pre_columns=seen)
    assert info["start_replaced"] == 0
    assert info["mass_columns"] == 0 or with_mass


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("name", ["poisson", "elast"])
def test_lobpcg_needs_no_more_iterations_than_pinvit(name, with_mass):
    it_p = ec.host_run(name, KIND[name], False, with_mass)[2]["iterations"]
    it_l = ec.host_run(name, KIND[name], True, with_mass)[2]["iterations"]
    print(f"{name}: PINVIT {it_p}, LOBPCG {it_l}")
    assert it_l <= it_p


def test_one_operator_product_per_iteration():
    """only A W is computed as a product: num columns for the start block, then the active columns once per iteration (+ the
    refresh of A X every 20 iterations)"""
    lams, X, info, seen = ec.host_run("poisson", "jacobi", True, False)
    its = info["iterations"]
    refresh = sum(int(np.sum((info["locked_at"] < 0) | (info["locked_at"] >= it))) for it in range(20, its + 1, 20))
    assert info["op_columns"] == ec.NUM["poisson"] + info["pre_columns"] + refresh


def test_equal_start_columns_fall_back_and_converge():
    name = "poisson"
    _, _, A, free = ec.problem(name)
    X0 = np.array(ec.start_block(name))
    X0[2] = X0[0]
    pre = ec.host_cycle(name, "jacobi")
    lams, X, info = lobpcg(ec.HostCSR(A), pre, ec.NUM[name], free=free, X0=HostMultiVector(X0), tol=ec.TOL, maxit=ec.MAXIT)
    assert info["start_replaced"] == 1
    ec.check_result(name, lams, X.data, info, False, pre_columns=pre.columns)


def test_exact_eigenvectors_return_at_iteration_zero():
    name = "poisson"
    _, _, A, free = ec.problem(name)
    num = ec.NUM[name]
    idx = np.flatnonzero(free)
    import scipy.sparse.linalg as spla
    lam, V = spla.eigsh(A[idx][:, idx].tocsc(), k=num, sigma=0.0, which="LM", tol=0)
    X0 = np.zeros((num, A.shape[0]))
    X0[:, idx] = V[:, np.argsort(lam)].T
    pre = ec.host_cycle(name, "jacobi")
    lams, X, info = lobpcg(ec.HostCSR(A), pre, num, free=free, X0=HostMultiVector(X0), tol=ec.TOL, maxit=ec.MAXIT)
    assert info["iterations"] == 0 and info["converged"] and pre.columns == 0
    assert np.all(info["locked_at"] == 0)
    assert np.allclose(lams, np.sort(lam), rtol=1e-12)


def test_maxit_is_not_an_error():
    name = "poisson"
    _, _, A, free = ec.problem(name)
    pre = ec.host_cycle(name, "jacobi")
    lams, X, info = lobpcg(ec.HostCSR(A), pre, ec.NUM[name], free=free, X0=HostMultiVector(np.array(ec.start_block(name))),
                           tol=1e-12, maxit=3)
    assert info["status"] == "maxit" and not info["converged"] and info["iterations"] == 3
    assert info["res"].shape == (4, ec.NUM[name]) and np.all(np.isfinite(lams))


def test_rank_deficient_basis_raises_nothing():
    """a preconditioner that returns the same direction for every column makes W rank deficient: the call stops and reports"""
    name = "poisson"
    _, _, A, free = ec.problem(name)

    class Same:
        def apply_block(self, X, Y):
            Y.data[...] = free * np.cos(np.arange(X.n))
    lams, X, info = lobpcg(ec.HostCSR(A), Same(), 3, free=free, X0=HostMultiVector(np.array(ec.start_block(name))[:3]), maxit=10)
    assert info["status"] in ("breakdown", "maxit") and not info["converged"]


def test_argument_errors():
    _, _, A, free = ec.problem("poisson")
    X0 = HostMultiVector(np.array(ec.start_block("poisson")))
    pre = ec.host_cycle("poisson", "jacobi")
    with pytest.raises(NgsAMGError, match="AMGX_MULTI_MAX"):
        lobpcg(ec.HostCSR(A), pre, 9, free=free, X0=X0)
    with pytest.raises(NgsAMGError, match="columns"):
        lobpcg(ec.HostCSR(A), pre, 2, free=free, X0=X0)
    with pytest.raises(NgsAMGError, match="X0"):
        lobpcg(ec.HostCSR(A), pre, 2, free=free)
