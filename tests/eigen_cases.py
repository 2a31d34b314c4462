"""Shared pieces of the eigensolver tests (tests/test_eigen_cpu.py, tests/test_gpu_eigen.py): the two problems, their reference
spectra, host-side block operators and the checks every result has to pass.

Problems (non-cubic grids: a cube's degenerate eigenvalues are the classic way to make LOBPCG look broken):
    "poisson"  poisson_case((17, 13, 11), Dirichlet "right|top"), scalar
    "elast"    elasticity_case((7, 7, 7)), 3x3 blocks, clamped left
Reference: scipy.sparse.linalg.eigsh in shift-invert mode on the free-free submatrix, NUM + 1 eigenvalues; the tests assert a
relative gap (lambda_{NUM+1} - lambda_NUM) / lambda_NUM >= 0.05 -- a condition on the input, not a measurement.

Lumped mass: a diagonal M with entries in [0.5, 1], largest entry exactly 1.  For r = A x - theta M x the Krylov-Weinstein bound
is  min_i |theta - lambda_i| <= |r|_{M^-1} / |x|_M <= |M^-1/2| |r|_2 |M^1/2| / |M x|_2 = res |theta| |M^-1/2| |M^1/2|  with
res = |r|_2 / (|theta| |M x|_2); |M^1/2| = 1 here, so kappa = |M^-1/2| (1 without a mass matrix)."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from ngsamg_amd.multivector import HostMultiVector
from tests.cheby_ref import ChebyRef, power_estimate
from tests.problems import elasticity_case, poisson_case

NUM = {"poisson": 4, "elast": 3}
TOL = 1e-8
MAXIT = 120
GAP = 0.05


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == "poisson":
        p, H = poisson_case((17, 13, 11), "right|top", 20)
    else:
        p, H = elasticity_case((7, 7, 7), False, 20)
    A = H.levels[0].A.to_scipy().tocsr()
    free = np.repeat(np.asarray(p.free, dtype=np.float64), p.bs)
    return p, H, A, free


@functools.lru_cache(maxsize=None)
def lmax(name):
    H = problem(name)[1]
    return tuple(1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]) + (1.0,)


@functools.lru_cache(maxsize=None)
def mass_diag(name):
    n = problem(name)[2].shape[0]
    m = 0.75 + 0.25 * np.cos(0.37 * np.arange(n))
    m[0] = 1.0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(name, with_mass):
    """(lambda_1 .. lambda_{NUM+1}, a bound of their own error): the reference's Krylov-Weinstein bound from its residuals"""
    _, _, A, free = problem(name)
    idx = np.flatnonzero(free)
    Aff = A[idx][:, idx].tocsc()
    k = NUM[name] + 1
    if with_mass:
        m = mass_diag(name)[idx]
        lam, V = spla.eigsh(Aff, k=k, M=sp.diags(m).tocsc(), sigma=0.0, which="LM", tol=0)
    else:
        m = np.ones(idx.size)
        lam, V = spla.eigsh(Aff, k=k, sigma=0.0, which="LM", tol=0)
    order = np.argsort(lam)
    lam, V = lam[order], V[:, order]
    R = Aff @ V - (m[:, None] * V) * lam
    err = np.linalg.norm(R, axis=0) / np.linalg.norm(m[:, None] * V, axis=0) / np.sqrt(m.min())
    return lam, err


def assert_gap(name, with_mass):
    lam, _ = reference(name, with_mass)
    num = NUM[name]
    gap = (lam[num] - lam[num - 1]) / lam[num - 1]
    assert gap >= GAP, f"{name}: relative gap {gap:.3f} after eigenvalue {num}: choose another shape or num"


# ---- block operators (apply_block) that work on both backends -------------------------------------------------------------

class DiagMass:
    def __init__(self, name):
        self.m = np.array(mass_diag(name))
        self._dev = None
        self.kappa = 1.0 / np.sqrt(self.m.min())      # |M^-1/2| (and |M^1/2| = 1)

    def apply_block(self, X, Y):
        if hasattr(X.data, "is_cuda"):
            import torch
            if self._dev is None:
                self._dev = torch.from_numpy(self.m).to(X.data.device)
            torch.mul(X.data, self._dev, out=Y.data)
        else:
            np.multiply(X.data, self.m, out=Y.data)


class HostCSR:
    def __init__(self, A):
        self.A = A

    def apply_block(self, X, Y):
        Y.data[...] = (self.A @ X.data.T).T


class HostCycle:
    """a host preconditioner with apply(b) (the oracle, ChebyRef) as a block operator; counts the columns it sees"""

    def __init__(self, ref):
        self.ref = ref
        self.columns = 0

    def apply_block(self, X, Y):
        self.columns += X.k
        for j in range(X.k):
            Y.data[j] = self.ref.apply(np.array(X.data[j]))


def host_cycle(name, kind):
    """the CPU twin of a device smoother: "jacobi" / "gs" = the oracle's V(1,1) cycle, "cheby" = ChebyRef with the fixed lambda_max"""
    H = problem(name)[1]
    if kind == "cheby":
        return HostCycle(ChebyRef(H, sm="cheby", degree=2, lambda_max=list(lmax(name))))
    from oracle.pyoracle import Oracle
    return HostCycle(Oracle(H.levels, sm_type={"jacobi": "jacobi", "gs": "gs_mc"}[kind]))


@functools.lru_cache(maxsize=None)
def start_block(name, seed=3):
    n = problem(name)[2].shape[0]
    X = np.random.default_rng(seed).standard_normal((NUM[name], n))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def host_run(name, kind, history, with_mass):
    """lobpcg on the numpy backend, once per configuration: (lams, X (k, n) array, info, columns the preconditioner saw)"""
    from ngsamg_amd.eigen import lobpcg
    _, _, A, free = problem(name)
    pre = host_cycle(name, kind)
    mass = DiagMass(name) if with_mass else None
    lams, X, info = lobpcg(HostCSR(A), pre, NUM[name], mass=mass, free=free, X0=HostMultiVector(np.array(start_block(name))),
                           tol=TOL, maxit=MAXIT, history=history)
    return lams, X.data, info, pre.columns


def true_residuals(name, lams, X, with_mass):
    """res_j of the returned pairs, recomputed from X with the host matrix"""
    _, _, A, free = problem(name)
    m = mass_diag(name) if with_mass else np.ones(A.shape[0])
    MX = X * m
    R = ((A @ X.T).T - lams[:, None] * MX) * free
    return np.linalg.norm(R, axis=1) / (np.abs(lams) * np.linalg.norm(MX, axis=1))


def check_result(name, lams, X, info, with_mass, pre_columns=None):
    """the checks of a converged run; X: (k, n) numpy array.  Returns the per-column bounds on |theta - lambda|."""
    num = NUM[name]
    _, _, A, free = problem(name)
    lam, ref_err = reference(name, with_mass)
    kappa = DiagMass(name).kappa if with_mass else 1.0
    m = mass_diag(name) if with_mass else np.ones(A.shape[0])
    print(f"{name}: iterations {info['iterations']} locked_at {info['locked_at']} theta {lams} restarts {info['restarts']} "
          f"joint {info['joint_orth']}")
    assert info["converged"] and info["status"] == "converged"
    assert info["iterations"] < MAXIT
    assert np.all(info["locked_at"] >= 0) and np.all(info["locked_at"] <= info["iterations"])
    assert info["res"].shape == (info["iterations"] + 1, num)
    assert not np.any(X * (1.0 - free)), "non-free rows must stay zero"
    res = true_residuals(name, lams, X, with_mass)
    print("  residuals (returned pairs, recomputed):", res, " reported:", info["res"][-1])
    assert np.all(res <= 1.01 * TOL)
    # Krylov-Weinstein, with res the residual in exactly that scaling (module docstring) + the reference's own error
    bound = res * np.abs(lams) * kappa + ref_err[:num] * kappa
    print("  |theta - lambda|:", np.abs(lams - lam[:num]), " bound:", bound)
    assert np.all(np.abs(lams - lam[:num]) <= bound)
    G = X @ (m * X).T
    assert np.max(np.abs(G - np.eye(num))) <= 1e-10
    # locked columns get no further preconditioner work: per iteration exactly the columns not yet locked
    if pre_columns is not None:
        expect = sum(int(np.sum((info["locked_at"] < 0) | (info["locked_at"] > it))) for it in range(info["iterations"]))
        assert pre_columns == expect == info["pre_columns"]
    return bound
