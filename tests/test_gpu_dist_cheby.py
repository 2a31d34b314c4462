"""Chebyshev smoother on rank-partitioned hierarchies: virtual ranks on ONE GPU (LoopbackComm) through
amgx_dist_*, checked against tests/cheby_ref.py::ChebyRef on the assembled global hierarchy with the device's lambda_max values.
The recurrence does not depend on the order of the rows, so the rank-partitioned cycle is the serial cycle up to rounding: 1e-12
relative, the bound of the rank-partitioned Jacobi tests against the oracle and of the single-rank Chebyshev tests against
ChebyRef."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, (16, 16, 16), 3, 200), (4, (12, 12, 12), 3, 100), (4, (40, 40), 2, 100), (3, (20, 9, 9), 3, 100), (1, (20, 18, 16), 3, 200)]


def _pgrid(R, dim):
    from ngsamg_amd import dist as D
    return (R, 1, 1) if R == 3 else D.proc_grid(R, dim)


def _poisson(R, box, dim, dmin, pg=None, **kw):
    from ngsamg_amd import dist as D
    pg = pg or _pgrid(R, dim)
    kw.setdefault("cheb_degree", 2)
    states = [D.assemble_poisson_owned(r, pg, box) for r in range(R)]
    return D.DistributedAMG(D.LoopbackComm(R), states, dim=dim, dist_min_rows=dmin, device=0, max_coarse_size=10, sm_type="cheby", **kw)


def _ref(amg, **kw):
    """the serial Chebyshev cycle on the assembled global hierarchy, with the intervals the device uses"""
    from tests.cheby_ref import ChebyRef
    glv = amg.global_levels()
    lam = [amg.smoother_info(l)["lambda_max"] if l + 1 < len(glv) else 1.0 for l in range(len(glv))]
    n = int(amg.tail_hier.coarse_n)
    cinv = np.asarray(amg.tail_hier.coarse_inv, dtype=np.float64).reshape(n, n) if n else None
    return ChebyRef(glv, sm="cheby", degree=amg.cheb_degree, ratio=amg.cheb_ratio, lambda_max=lam, coarse_inv=cinv, **kw)


def _rhs(amg, seed=0):
    import torch
    sts = amg.dist_levels[0]
    rng = np.random.default_rng(seed)
    bs0 = int(getattr(sts[0], "bs", 1))
    bh = [rng.standard_normal(s.n * bs0) * np.repeat(s.free, bs0) for s in sts]
    bs = [torch.from_numpy(b).cuda() for b in bh]
    xs = [torch.full((s.n * bs0,), float("nan"), dtype=torch.float64, device="cuda") for s in sts]
    return bh, bs, xs


def _cat(xs):
    return np.concatenate([x.cpu().numpy() for x in xs])


def _rel(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def _check_three_applications(amg, tol=1e-12, **refkw):
    """direct launches, capture, replay: each from a NaN-filled x"""
    import torch
    bh, bs, xs = _rhs(amg)
    ref = _ref(amg, **refkw).apply(np.concatenate(bh))
    for rep in range(3):
        for x in xs:
            x.fill_(float("nan"))
        amg.Mult(bs, xs)
        torch.cuda.synchronize()
        err = _rel(_cat(xs), ref)
        print(f"application {rep}: rel.err vs ChebyRef = {err:.3e}")
        assert err <= tol, (rep, err)


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("R,box,dim,dmin", CASES)
def test_cycle_matches_serial_chebyshev_cycle(R, box, dim, dmin, degree):
    amg = _poisson(R, box, dim, dmin, cheb_degree=degree)
    assert amg.k == 2
    _check_three_applications(amg)
    gi = amg._dev.graph_info()
    assert gi["enabled"] and gi["graphs"] == 1 and gi["replays"] == 2, gi


@pytest.mark.parametrize("R,box,dim,dmin", CASES[:4])
def test_collective_lambda_max_estimate(R, box, dim, dmin):
    """the estimator of amgx_create on the partitioned operator: same start vector (the fill at every rank's local index), same 30
    steps; a lower bound of lambda_max times 1.1"""
    import torch
    from tests.cheby_ref import fill_vector, lambda_true, power_estimate
    amg = _poisson(R, box, dim, dmin)
    glv = amg.global_levels()
    for l in range(amg.k):
        info = amg.smoother_info(l)                 # (asserts that the local ranks agree)
        assert info["sm_type"] == "cheby" and info["estimated"] == 1 and info["degree"] == 2
        lam = info["lambda_max"]
        v0 = np.concatenate([fill_vector(s.n, 1) for s in amg.dist_levels[l]])
        est = 1.1 * power_estimate(glv[l], 30, v0=v0)
        true = lambda_true(glv[l])
        print(f"level {l}: lambda = {lam:.15g}  restated = {est:.15g}  true = {true:.15g}  lambda / true = {lam / true:.4f}")
        assert abs(lam - est) <= 1e-10 * lam
        assert true <= lam <= 1.1 * true * (1 + 1e-10)
        assert abs(info["lambda_min"] - lam / 10.0) <= 1e-15 * lam
    for l in range(amg.k, len(glv) - 1):
        assert amg.smoother_info(l)["estimated"] == 1
    # the work vectors are clean: the first application after the estimate is right
    bh, bs, xs = _rhs(amg, 5)
    amg.Mult(bs, xs)
    torch.cuda.synchronize()
    assert _rel(_cat(xs), _ref(amg).apply(np.concatenate(bh))) <= 1e-12


def test_explicit_lambda_max_is_taken():
    amg = _poisson(2, (16, 16, 16), 3, 200, cheb_lambda_max=[1.9, 2.1])
    for l, v in enumerate([1.9, 2.1]):
        info = amg.smoother_info(l)
        assert info["estimated"] == 0 and info["lambda_max"] == v
    _check_three_applications(amg)


@pytest.mark.parametrize("R,box,rot", [(2, (8, 7, 7), False), (2, (6, 6, 5), True)])
def test_elasticity_block_levels(R, box, rot):
    from ngsamg_amd import dist as D
    pg = D.proc_grid(R, 3)
    states = [D.assemble_elasticity_owned(r, pg, box, rotations=rot) for r in range(R)]
    amg = D.DistributedAMG(D.LoopbackComm(R), states, dim=3, dist_min_rows=10, device=0, max_coarse_size=5, energy=1,
                           regularize_cmats=0 if rot else 1, sm_type="cheby", cheb_degree=2)
    assert all(amg.smoother_info(l)["estimated"] == 1 for l in range(amg.k))
    _check_three_applications(amg)


@pytest.mark.parametrize("R,box,dim,dmin", [CASES[0], CASES[2]])
@pytest.mark.parametrize("steps,symm,cycle", [(2, False, "V"), (1, True, "V"), (1, False, "W")])
def test_stepwise_driver(R, box, dim, dmin, steps, symm, cycle):
    amg = _poisson(R, box, dim, dmin, sm_steps=steps, sm_symm=symm, mg_cycle=cycle)
    _check_three_applications(amg, sm_steps=steps, sm_symm=symm, cycle=cycle)


@pytest.mark.parametrize("R,box,dim,dmin,degree", [(2, (16, 16, 16), 3, 200, 3), (4, (40, 40), 2, 100, 2)])
def test_overlap_and_graph_do_not_change_a_bit(R, box, dim, dmin, degree, monkeypatch):
    """interior rows beside the exchange + boundary rows after it == everything after it; graph replay == direct launches, also
    for new contents of the same b storage"""
    import torch

    def build(graph, no_overlap):
        monkeypatch.setenv("AMGX_DIST_GRAPH", "1" if graph else "0")
        if no_overlap:
            monkeypatch.setenv("AMGX_DIST_NO_OVERLAP", "1")
        else:
            monkeypatch.delenv("AMGX_DIST_NO_OVERLAP", raising=False)
        return _poisson(R, box, dim, dmin, cheb_degree=degree)
    ag, ad, an = build(True, False), build(False, False), build(False, True)
    sts = ag.dist_levels[0]
    assert any(s.n_interior > 0 for s in sts)
    rng = np.random.default_rng(3)
    bs = [torch.from_numpy(rng.standard_normal(s.n) * s.free).cuda() for s in sts]
    xg, xd, xn = ([torch.full((s.n,), float("nan"), dtype=torch.float64, device="cuda") for s in sts] for _ in range(3))
    for it in range(4):
        if it == 3:           # new right-hand side in the same storage: the captured graph must see it
            for b, s in zip(bs, sts):
                b.copy_(torch.from_numpy(rng.standard_normal(s.n) * s.free))
        ag.Mult(bs, xg)
        ad.Mult(bs, xd)
        an.Mult(bs, xn)
        torch.cuda.synchronize()
        for a, b_, c_ in zip(xg, xd, xn):
            assert torch.equal(a, b_) and torch.equal(a, c_)
    gi, di = ag._dev.graph_info(), ad._dev.graph_info()
    assert gi["enabled"] and gi["graphs"] == 1 and gi["replays"] == 3, gi
    assert not di["enabled"] and di["replays"] == 0
    assert ag._dev.n_exchanges() == ad._dev.n_exchanges() == an._dev.n_exchanges()


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_exchange_budget(degree, monkeypatch):
    """2 * degree exchanges per rank-partitioned level and application (degree 1: the literal Jacobi count)"""
    import torch
    monkeypatch.setenv("AMGX_DIST_GRAPH", "0")
    amg = _poisson(2, (16, 16, 16), 3, 200, cheb_degree=degree)
    bh, bs, xs = _rhs(amg)
    n0 = amg._dev.n_exchanges()
    amg.Mult(bs, xs)
    torch.cuda.synchronize()
    used = amg._dev.n_exchanges() - n0
    assert used <= 2 * degree * amg.k
    assert used == 2 * degree * amg.k


def test_rank_without_rows():
    """a rank that owns nothing takes part in the collective estimate (same branch, same interval) and in the cycle"""
    import scipy.sparse as sp
    from ngsamg_amd import bridge as B, dist as D
    pgrid, gshape = (2, 2, 1), (17, 17, 9)
    R = 5
    comm = D.LoopbackComm(R)
    locs = []
    for r in range(R - 1):
        L, _ = B.shared_poisson_partition(r, pgrid, gshape)
        L.rank = r + 1
        L.dist_procs = [np.asarray(p) + 1 for p in L.dist_procs]
        locs.append(L)
    empty = B.SharedLocal(0, sp.csr_matrix((0, 0)), [], free=np.zeros(0, dtype=np.uint8), coords=np.zeros((0, 3)))
    states, vmaps = B.from_shared_layout(comm, [empty] + locs)
    assert states[0].n == 0
    amg = D.DistributedAMG(comm, states, dim=3, dist_min_rows=60, device=0, max_coarse_size=10, sm_type="cheby", cheb_degree=2)
    assert all(amg.smoother_info(l)["estimated"] == 1 for l in range(amg.k))
    _check_three_applications(amg)


@pytest.mark.parametrize("R,box,dmin", [(2, (14, 12, 12), 100), (4, (10, 10, 10), 50)])
def test_krylov_solvers_equal_the_serial_reference(R, box, dmin):
    import torch
    amg = _poisson(R, box, 3, dmin, pg=(R, 1, 1))
    bh, bs, _ = _rhs(amg, 7)
    sts = amg.dist_levels[0]
    xs = [torch.zeros(s.n, dtype=torch.float64, device="cuda") for s in sts]
    it, errs = amg.pcg(bs, xs, tol=1e-8, maxsteps=100)
    torch.cuda.synchronize()
    xo, ito, erro = _ref(amg).pcg(np.concatenate(bh), tol=1e-8, maxit=100)
    print(f"pcg: iterations {it} (reference {ito})")
    assert it == ito and it < 60
    erro = np.asarray(erro)[:it + 1]
    assert np.all(np.abs(errs - erro) <= 1e-6 * erro[0])
    assert _rel(_cat(xs), xo) <= 1e-8
    xg = [torch.zeros(s.n, dtype=torch.float64, device="cuda") for s in sts]
    itg, errg = amg.gmres(bs, xg, tol=1e-10, maxsteps=100)
    torch.cuda.synchronize()
    assert 0 < itg < 100
    assert _rel(_cat(xg), xo) <= 1e-7


def _patched_desc(monkeypatch, change):
    """hierarchy_desc whose descriptor of the rank-partitioned levels (clev = none) is changed before amgx_dist_create sees it"""
    from ngsamg_amd import device as dev
    orig = dev.hierarchy_desc

    def patched(h, **kw):
        out = orig(h, **kw)
        if kw.get("clev") == "none":
            change(out[0])
        return out
    monkeypatch.setattr(dev, "hierarchy_desc", patched)


def test_refusals(monkeypatch):
    from ngsamg_amd import dist as D
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import NgsAMGError
    states = lambda: [D.assemble_poisson_owned(r, (2, 1, 1), (16, 16, 16)) for r in range(2)]
    kw = dict(dim=3, dist_min_rows=200, device=0, max_coarse_size=10, sm_type="cheby", cheb_degree=2)
    with pytest.raises(NgsAMGError, match="explicit cheb_degree"):         # the type alone: refused, the degree has no default
        D.DistributedAMG(D.LoopbackComm(2), states(), **dict(kw, cheb_degree=None))
    with pytest.raises(NgsAMGError, match="device driver only"):
        D.DistributedAMG(D.LoopbackComm(2), states(), backend=lambda top, tail, i: None, **kw)
    amg = D.DistributedAMG(D.LoopbackComm(2), states(), **kw)
    assert amg.k == 2
    amg.fold = True                                   # fold with Chebyshev at the C ABI
    with pytest.raises(NgsAMGError, match="fold"):
        D._DeviceDist(amg, 0)
    amg.fold = False
    with monkeypatch.context() as m:                  # a descriptor without the opt-in
        m.setattr(_lib.amgx_dist_desc, "cheby", property(lambda self: 0, lambda self, v: None))
        with pytest.raises(NgsAMGError, match="opt-in"):
            D._DeviceDist(amg, 0)
    with monkeypatch.context() as m:
        _patched_desc(m, lambda d: setattr(d.levels[1], "mat_prec", 1))
        with pytest.raises(NgsAMGError, match="level 1.*AMGX_PREC_F32"):
            D._DeviceDist(amg, 0)
    with monkeypatch.context() as m:
        _patched_desc(m, lambda d: setattr(d.levels[1], "cheb_degree", 3))
        with pytest.raises(NgsAMGError, match="same cheb_degree"):
            D._DeviceDist(amg, 0)


def test_rccl_world_size_one_chebyshev():
    """degree 2 with an estimated interval through a real RCCL communicator at world size 1 (child process with its own watchdog):
    the collective estimate, the cycle against ChebyRef, the whole-cycle graph captured and replayed"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NGSAMG_CHECK_TIMEOUT="200")
    r = subprocess.run(["timeout", "-k", "10", "280", sys.executable, os.path.join(root, "tests", "dist_rccl_cheby_check.py"), "--box", "20"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "RCCL CHEBY CHECK PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "estimated = 1" in r.stdout and "graph enabled = True graphs = 1 replays = 2" in r.stdout, r.stdout
