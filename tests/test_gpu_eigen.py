"""ngsamg_amd.eigen.lobpcg on device handles: the problems, bounds and locking checks of tests/test_eigen_cpu.py (shared through
tests/eigen_cases.py), with A = MatVecMulti(0, dev) and the preconditioner MultMulti(dev).

Poisson: sm_type "jacobi" (the fused multi-vector handle) and "gs" (the column-loop handle); elasticity: sm_type "cheby" with
fuse=False and fuse=True.  PINVIT and LOBPCG, identity and lumped mass.  The iteration count on the device is at most
ceil(1.15 x the count of the numpy backend) on the same problem and start block with the CPU twin of the smoother as
preconditioner (the project's allowance for a parallel order against the sequential one); the numpy count is computed
here, not hard-coded."""
import functools
import math

import numpy as np
import pytest
import torch

from ngsamg_amd.eigen import lobpcg
from ngsamg_amd.multivector import DeviceMultiVector, MatVecMulti, MultMulti
from tests import eigen_cases as ec

pytestmark = pytest.mark.gpu

CONFIGS = [("poisson", "jacobi", False), ("poisson", "gs", False), ("elast", "cheby", False), ("elast", "cheby", True)]
IDS = ["poisson-jacobi", "poisson-gs", "elast-cheby", "elast-cheby-fuse"]


@functools.lru_cache(maxsize=None)
def _dev(name, kind):
    from ngsamg_amd.device import DeviceAMGMatrix
    H = ec.problem(name)[1]
    kw = dict(cheb_degree=2, cheb_lambda_max=list(ec.lmax(name))) if kind == "cheby" else {}
    return DeviceAMGMatrix(H, sm_type=kind, **kw)


@functools.lru_cache(maxsize=None)
def _run(name, kind, fuse, history, with_mass):
    dev = _dev(name, kind)
    free = torch.from_numpy(ec.problem(name)[3]).cuda()
    A, pre = MatVecMulti(0, dev), MultMulti(dev)
    X0 = DeviceMultiVector(dev, torch.from_numpy(np.array(ec.start_block(name))).cuda())
    mass = ec.DiagMass(name) if with_mass else None
    lams, X, info = lobpcg(A, pre, ec.NUM[name], mass=mass, free=free, X0=X0, tol=ec.TOL, maxit=ec.MAXIT, history=history, fuse=fuse)
    assert isinstance(X, DeviceMultiVector)
    return lams, X.data.cpu().numpy(), info, pre.columns, A.columns


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("history", [False, True], ids=["pinvit", "lobpcg"])
@pytest.mark.parametrize("name,kind,fuse", CONFIGS, ids=IDS)
def test_eigenpairs_on_the_device(name, kind, fuse, history, with_mass):
    ec.assert_gap(name, with_mass)
    lams, X, info, pre_cols, op_cols = _run(name, kind, fuse, history, with_mass)
    ec.check_result(name, lams, X, info, with_mass, pre_columns=pre_cols)
    assert op_cols == info["op_columns"]
    host_its = ec.host_run(name, kind, history, with_mass)[2]["iterations"]
    print(f"iterations: device {info['iterations']}, numpy backend {host_its}")
    assert info["iterations"] <= math.ceil(1.15 * host_its)


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("name,kind,fuse", CONFIGS, ids=IDS)
def test_lobpcg_needs_no_more_iterations_than_pinvit(name, kind, fuse, with_mass):
    assert _run(name, kind, fuse, True, with_mass)[2]["iterations"] <= _run(name, kind, fuse, False, with_mass)[2]["iterations"]


@pytest.mark.parametrize("with_mass", [False, True], ids=["identity", "lumped"])
@pytest.mark.parametrize("history", [False, True], ids=["pinvit", "lobpcg"])
def test_fused_and_column_loop_agree(history, with_mass):
    """fuse=True and fuse=False: eigenvalues within the sum of their bounds"""
    name = "elast"
    a = _run(name, "cheby", False, history, with_mass)
    b = _run(name, "cheby", True, history, with_mass)
    ba = ec.check_result(name, a[0], a[1], a[2], with_mass)
    bb = ec.check_result(name, b[0], b[1], b[2], with_mass)
    assert np.all(np.abs(a[0] - b[0]) <= ba + bb)
    plan = _dev(name, "cheby").multi_plan(ec.NUM[name], fuse=True)
    assert plan["fused"] == 1, plan["note"]


def test_eigensolve_on_the_python_surface():
    """pre.EigenSolve next to pre.MultMulti: random start block, the hierarchy's free dofs"""
    from ngsamg_amd import NgsAMG
    name = "poisson"
    p, H, A, free = ec.problem(name)
    pre = NgsAMG.h1_scal(H.levels[0].A, p.free, p.coords, ngs_amg_sm_type="jacobi", ngs_amg_max_coarse_size=20)
    lams, X, info = pre.EigenSolve(ec.NUM[name], tol=ec.TOL, maxit=ec.MAXIT, seed=1)
    ec.check_result(name, lams, X.data.cpu().numpy(), info, False)
