"""Chebyshev polynomial smoother (sm_type "cheby", AMGX_SM_CHEBY) on the device against the numpy reference of
tests/cheby_ref.py, which tests/test_cheby_cpu.py ties to the oracle.

Tolerances: 1e-12 relative where only the summation order differs (cycles, smoothers), PCG iterations +-1,
histories to 1e-6, the estimator to 1e-10 against its numpy restatement."""
import os

import numpy as np
import pytest

from tests.cheby_ref import ChebyRef, lambda_true, power_estimate
from tests.problems import elasticity_case, poisson_case, rhs, to_matrix

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
ONE_LANE = {"AMGX_SELL_MAX_LANES": "1"}
NO_FUSE = {"AMGX_CHEB_NO_FUSED_RESTRICT": "1"}


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


def _lmax(H, steps=20):
    """explicit per-level interval ends, different on every level"""
    return [1.1 * power_estimate(lv, steps) for lv in H.levels[:-1]] + [1.0]


def _problems():
    return [("poisson2d 33^2", poisson_case((33, 33), "left|top", 5)),
            ("poisson2d 40x23", poisson_case((40, 23), "right", 10)),
            ("poisson3d 17^3", poisson_case((17, 17, 17), "right|top", 20)),
            ("poisson3d 9x30x13", poisson_case((9, 30, 13), ".*", 20)),
            ("poisson3d 25^3", poisson_case((25, 25, 25), "right|top", 20)),
            ("elasticity 3x3/6x6", elasticity_case((13, 11, 9), False, 5, 0.12)),
            ("elasticity 6x6/6x6", elasticity_case((13, 11, 9), True, 5, 0.12))]


def _mult(dev, b, device=False, graph=True):
    if device:
        import torch
        bd = torch.from_numpy(b).cuda()
        xd = torch.full_like(bd, float("nan"))
        dev.Mult(bd, xd, graph=graph)
        torch.cuda.synchronize()
        return xd.cpu().numpy()
    x = np.full_like(b, np.nan)
    dev.Mult(b, x, graph=graph)
    return x


# ---- 6. application against the numpy reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_cycle_matches_reference(cycle, degree):
    for name, (p, H) in _problems():
        lm = _lmax(H)
        b = rhs(p, 3)
        ref = ChebyRef(H, sm="cheby", degree=degree, lambda_max=lm, cycle=cycle).apply(b)
        for env in ((None, NO_DENSE) if cycle == "V" else (None,)):
            dev = _dev(H, env, sm_type="cheby", mg_cycle=cycle, cheb_degree=degree, cheb_lambda_max=lm)
            ci = dev.cycle_info()
            if env is NO_DENSE:
                assert ci["dense_level"] < 0, ci
            assert ci["tail_level"] < 0, ci                      # the single-workgroup tail does not take Chebyshev levels
            for l in range(H.n_levels - 1):
                si = dev.smoother_info(l)
                assert si["sm_type"] == "cheby" and si["degree"] == degree and si["estimated"] == 0, si
                assert si["lambda_max"] == lm[l] and abs(si["lambda_min"] - lm[l] / 10.0) <= 1e-15 * lm[l], si
            runs = [(False, True)] + ([(True, True), (True, False), (False, False)] if degree in (2, 3) else [])
            for device, graph in runs:
                e = _rel(_mult(dev, b, device, graph), ref)
                print(f"{name} {cycle} degree {degree} dense={ci['dense_level']} device={int(device)} graph={int(graph)}: {e:.2e}")
                assert e <= 1e-12, (name, cycle, degree, env, device, graph, e)
            if degree == 2:                                       # a replayed graph gives the same bits as its first launch
                import torch
                bd = torch.from_numpy(b).cuda()
                x1, x2 = torch.empty_like(bd), torch.empty_like(bd)
                dev.Mult(bd, x1)
                x1c = x1.clone()
                dev.Mult(bd, x1)
                dev.Mult(bd, x2)
                torch.cuda.synchronize()
                assert torch.equal(x1, x1c) and torch.equal(x1, x2)


@pytest.mark.parametrize("cycle", ["V", "W"])
def test_degree_one_uniform_lambda_matches_oracle_jacobi(cycle):
    from oracle.pyoracle import Oracle
    lmax = 2.2
    theta = 0.5 * (lmax + lmax / 10.0)
    for name, (p, H) in _problems():
        b = rhs(p, 4)
        ref = Oracle(H.levels, sm_type="jacobi", omega=1.0 / theta, cycle=cycle).apply(b)
        for env in (None, NO_DENSE):
            dev = _dev(H, env, sm_type="cheby", mg_cycle=cycle, cheb_degree=1, cheb_lambda_max=lmax)
            e = _rel(_mult(dev, b), ref)
            print(name, cycle, e)
            assert e <= 1e-12, (name, cycle, env, e)


def test_sm_steps_and_symm_compose_in_the_cycle():
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    pe, He = elasticity_case((13, 11, 9), True, 5, 0.12)
    for (pp, HH) in ((p, H), (pe, He)):
        lm = _lmax(HH)
        b = rhs(pp, 6)
        for steps, symm in ((2, False), (1, True), (2, True)):
            for cycle in ("V", "W"):
                ref = ChebyRef(HH, sm="cheby", degree=2, lambda_max=lm, cycle=cycle, sm_steps=steps, sm_symm=symm).apply(b)
                dev = _dev(HH, sm_type="cheby", mg_cycle=cycle, cheb_lambda_max=lm, sm_steps=steps, sm_symm=symm)
                e = _rel(_mult(dev, b), ref)
                print(HH.levels[0].bs, steps, symm, cycle, e)
                assert e <= 1e-12, (steps, symm, cycle, e)


# ---- 7. the flag contract of amgx_smooth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,symm", [(1, False), (2, False), (1, True), (2, True)])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_smoother_flag_contract(steps, symm, degree):
    import torch
    for name, (p, H) in (("poisson2d", poisson_case((33, 33), "left|top", 5)), ("poisson3d", poisson_case((17, 17, 17), "right|top", 20)),
                         ("elasticity 3x3/6x6", elasticity_case((13, 11, 9), False, 5, 0.12)),
                         ("elasticity 6x6", elasticity_case((13, 11, 9), True, 5, 0.12))):
        lm = _lmax(H)
        ref = ChebyRef(H, sm="cheby", degree=degree, lambda_max=lm, sm_steps=steps, sm_symm=symm)
        dev = _dev(H, sm_type="cheby", cheb_degree=degree, cheb_lambda_max=lm, sm_steps=steps, sm_symm=symm)
        rng = np.random.default_rng(5)
        for l in range(min(2, H.n_levels - 1)):
            n = dev.sizes[l]
            A = H.levels[l].A.to_scipy()
            free = np.repeat(np.asarray(H.levels[l].free), H.levels[l].bs)
            for back in (False, True):
                for ru in (False, True):
                    for ur in (False, True):
                        for xz in (False, True):
                            b = rng.standard_normal(n) * free
                            x = np.zeros(n) if xz else rng.standard_normal(n) * free
                            res = (b - A @ x) if ru else rng.standard_normal(n)
                            xr, rr = x.copy(), res.copy()
                            ref.smooth(l, xr, b, rr, ru, ur, xz, back)
                            xg, rg = x.copy(), res.copy()
                            dev.Smooth(l, xg, b, rg, ru, ur, xz, back)
                            ex, er = _rel(xg, xr), _rel(rg, rr)
                            assert ex <= 1e-12, (name, l, back, ru, ur, xz, ex)
                            if ur:
                                assert er <= 1e-12, (name, l, back, ru, ur, xz, er)
                            if l == 0 and not back:                       # device pointers
                                xd, bd, rd = (torch.from_numpy(v.copy()).cuda() for v in (x, b, res))
                                dev.Smooth(l, xd, bd, rd, ru, ur, xz, back)
                                torch.cuda.synchronize()
                                assert _rel(xd.cpu().numpy(), xr) <= 1e-12, (name, l, ru, ur, xz)
                                if ur:
                                    assert _rel(rd.cpu().numpy(), rr) <= 1e-12, (name, l, ru, ur, xz)


def test_smooth_v_from_level_matches_reference():
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    lm = _lmax(H)
    ref = ChebyRef(H, sm="cheby", degree=2, lambda_max=lm)
    dev = _dev(H, sm_type="cheby", cheb_lambda_max=lm)
    rng = np.random.default_rng(2)
    for l in range(H.n_levels - 1):
        n = dev.sizes[l]
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
        xr, rr = x0.copy(), np.zeros(n)
        ref.smooth_v_from_level(l, xr, b, rr, False, True, False)
        xg, rg = x0.copy(), np.zeros(n)
        dev.SmoothVFromLevel(l, xg, b, rg, False, True, False)
        assert _rel(xg, xr) <= 1e-12 and _rel(rg, rr) <= 1e-12, (l, _rel(xg, xr), _rel(rg, rr))


# ---- 8. the residual after pre-smoothing feeds the chunk-local restriction without going through HBM -----------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
def test_fused_residual_restriction(cycle):
    seen_lanes = set()
    for name, (p, H), env in (("poisson3d 25^3", poisson_case((25, 25, 25), "right|top", 20), {}),
                              ("poisson2d 33^2", poisson_case((33, 33), "left|top", 5), {}),
                              ("poisson2d 70x50, one lane", poisson_case((70, 50), "left|top", 5), ONE_LANE),
                              ("poisson3d 23x22x21, one lane", poisson_case((23, 22, 21), "right|top", 20), ONE_LANE)):
        lm = _lmax(H)
        b = rhs(p, 8)
        ref = ChebyRef(H, sm="cheby", degree=2, lambda_max=lm, cycle=cycle).apply(b)
        fused = _dev(H, dict(NO_DENSE, **env), sm_type="cheby", mg_cycle=cycle, cheb_lambda_max=lm)
        plain = _dev(H, dict(NO_DENSE, **env, **NO_FUSE), sm_type="cheby", mg_cycle=cycle, cheb_lambda_max=lm)
        lp = fused.level_paths(0)
        print(name, cycle, {k: lp[k] for k in ("kernel", "fused_block", "lanes", "ept", "compact", "chunks")}, fused.matrix_info(0, "A"))
        assert lp["kernel"] == "cheby-res" and lp["fused_block"] == 512 and lp["chunks"] > 0, lp
        assert fused.matrix_info(0, "A")["fmt"] == "sell" and fused.matrix_info(0, "A")["lanes"] == lp["lanes"]
        seen_lanes.add(lp["lanes"])
        for l in range(H.n_levels):
            assert plain.level_paths(l)["kernel"] is None, (name, l)
        xf, xp = _mult(fused, b), _mult(plain, b)
        assert _rel(xf, ref) <= 1e-12 and _rel(xp, ref) <= 1e-12 and _rel(xf, xp) <= 1e-12, (name, _rel(xf, ref), _rel(xp, ref))
        assert _rel(_mult(fused, b, device=True, graph=True), ref) <= 1e-12
        # block levels keep EP_RES + the restriction kernels
    assert 1 in seen_lanes and any(g > 1 for g in seen_lanes), seen_lanes
    pe, He = elasticity_case((13, 11, 9), True, 5, 0.12)
    de = _dev(He, sm_type="cheby", mg_cycle=cycle)
    assert all(de.level_paths(l)["kernel"] is None for l in range(He.n_levels))


# ---- 9. the estimator ------------------------------------------------------------------------------------------------------
def _estimator_cases():
    return [("poisson 24^3", poisson_case((24, 24, 24), "right|top", 20)),
            ("elasticity 10^3 displacements", elasticity_case((10, 10, 10), False, 20)),
            ("elasticity 10^3 rotations", elasticity_case((10, 10, 10), True, 20)),
            ("elasticity 14^3 rotations", elasticity_case((14, 14, 14), True, 20))]


def test_lambda_max_estimate():
    for name, (p, H) in _estimator_cases():
        dev = _dev(H, sm_type="cheby")
        for l, lv in enumerate(H.levels[:-1]):
            si = dev.smoother_info(l)
            assert si["estimated"] == 1 and si["degree"] == 2, si
            want = 1.1 * power_estimate(lv, 30)
            true = lambda_true(lv)
            print(f"{name} level {l} n {lv.n} bs {lv.bs}: device {si['lambda_max']:.12f} numpy {want:.12f} true {true:.12f} "
                  f"ratio {si['lambda_max'] / true:.4f}")
            assert abs(si["lambda_max"] - want) <= 1e-10 * want, (name, l, si, want)
            assert abs(si["lambda_min"] - si["lambda_max"] / 10.0) <= 1e-15 * want
            assert true <= si["lambda_max"] <= 1.1 * true * (1 + 1e-10), (name, l, si["lambda_max"], true)
        # the work vectors the estimate used are clean again: the first application is right
        lm = [dev.smoother_info(l)["lambda_max"] for l in range(H.n_levels - 1)] + [1.0]
        b = rhs(p, 1)
        assert _rel(_mult(dev, b), ChebyRef(H, sm="cheby", degree=2, lambda_max=lm).apply(b)) <= 1e-12


# ---- 10. the solver through the preconditioner classes ---------------------------------------------------------------------
def _pcg_parity(c, p, H, b, tol, budget=None):
    from ngsamg_amd.krylov import NativeCGSolver
    dev = c.GetAMGMatrix()._dev
    n = H.n_levels
    lm = [dev.smoother_info(l)["lambda_max"] for l in range(n - 1)] + [1.0]
    assert all(dev.smoother_info(l)["sm_type"] == "cheby" and dev.smoother_info(l)["estimated"] == 1 for l in range(n - 1))
    _, it_ref, errs_ref = ChebyRef(H, sm="cheby", degree=2, lambda_max=lm).pcg(b, tol=tol, maxit=100)
    cg = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
    cg.Solve(b)
    print("pcg iterations: device", cg.iterations, "reference", it_ref)
    assert abs(cg.iterations - it_ref) <= 1, (cg.iterations, it_ref)
    m = min(cg.iterations, it_ref) + 1
    assert np.allclose(np.asarray(cg.errors[:m]), errs_ref[:m], rtol=1e-6, atol=0), (cg.errors[:m], errs_ref[:m])
    if budget is not None:
        assert cg.iterations <= budget, cg.iterations
    lmin, lmx, kappa = c.Test()
    print("Test():", lmin, lmx, kappa)
    assert 0.0 < lmin <= lmx <= 1.0 + 1e-8 and kappa < 50.0          # lambda(C A) <= 1: the smoother cannot diverge
    return cg.iterations


def test_solver_h1_3d():
    from ngsamg_amd import NgsAMG, fem, Matrix
    p = fem.poisson_fast((15, 15, 15), dirichlet="left|top")
    val = p.val[:, None, None] * np.eye(3)[None]
    A = Matrix(p.n, p.n, 3, 3, p.rowptr, p.col, val)
    c = NgsAMG.h1_3d(A, p.free, ngs_amg_max_coarse_size=10, ngs_amg_sm_type="cheby")
    b = np.repeat(p.load, 3) * np.tile(np.arange(1, 4), p.n)
    _pcg_parity(c, p, c.GetHierarchy(), b, 1e-8)


@pytest.mark.parametrize("rot", [False, True])
def test_solver_elast_3d(rot):
    from ngsamg_amd import NgsAMG, fem
    p = fem.elasticity_fast((10, 10, 10), dirichlet="left", mu=1.0, lam=0.5, rotations=rot)
    c = NgsAMG.elast_3d(to_matrix(p), p.free, coords=p.coords, ngs_amg_max_coarse_size=20, ngs_amg_sm_type="cheby")
    _pcg_parity(c, p, c.GetHierarchy(), np.ascontiguousarray(p.load, dtype=np.float64), 1e-8)
    if rot:
        # the budget of tests/test_cheby_cpu.py: degree 1 within 20 iterations where block Jacobi (omega = 0.9) needs > 100
        from ngsamg_amd.krylov import NativeCGSolver
        c1 = NgsAMG.elast_3d(to_matrix(p), p.free, coords=p.coords, ngs_amg_max_coarse_size=20, ngs_amg_sm_type="cheby", ngs_amg_cheb_degree=1)
        d1 = c1.GetAMGMatrix()._dev
        assert d1.smoother_info(0)["degree"] == 1
        cg = NativeCGSolver(d1, d1, tol=1e-8, maxsteps=100)
        cg.Solve(np.ascontiguousarray(p.load, dtype=np.float64))
        print("rotations, degree 1:", cg.iterations)
        assert cg.iterations <= 20 and cg.errors[-1] <= 1e-8 * cg.errors[0], cg.iterations


# ---- 11. edges -------------------------------------------------------------------------------------------------------------
def test_multi_vector_calls_take_the_column_loop():
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, sm_type="cheby", cheb_lambda_max=_lmax(H))
    B = np.stack([rhs(p, j) for j in range(5)])
    for k in (1, 2, 5):
        info = dev.multi_info(k)
        assert info["fused"] == 0 and info["groups"] == [1] * k, info
        X = np.full_like(B[:k], np.nan)
        dev.MultMulti(np.ascontiguousarray(B[:k]), X)
        for j in range(k):
            xj = np.empty(p.n)
            dev.Mult(np.ascontiguousarray(B[j]), xj)
            assert np.array_equal(X[j], xj), (k, j)


def test_errors():
    import ctypes as C
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = poisson_case((33, 33), "left|top", 5)
    with pytest.raises(_lib.NgsAMGError, match="1 .. 8"):
        _dev(H, sm_type="cheby", cheb_degree=9)
    lib = _lib.hip()
    for field, value, msg in (("cheb_degree", 9, "cheb_degree"), ("cheb_degree", -1, "cheb_degree"), ("cheb_lambda_max", -1.0, "cheb_lambda_max"),
                              ("cheb_ratio", 1.0, "cheb_ratio"), ("cheb_ratio", -2.0, "cheb_ratio")):
        desc, keep, _ = hierarchy_desc(H, sm_type="cheby")
        setattr(desc.levels[0], field, value)
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, (field, value)
        assert msg in lib.amgx_last_error(None).decode(), lib.amgx_last_error(None).decode()
    dev = _dev(H, sm_type="jacobi")
    with pytest.raises(_lib.NgsAMGError, match="Chebyshev"):
        dev.time_op(0, 10)
    assert dev.smoother_info(0) == {"sm_type": "jacobi", "degree": 0, "lambda_max": 0.0, "lambda_min": 0.0, "estimated": 0}
    ch = _dev(H, sm_type="cheby")
    assert ch.time_op(0, 10, reps=3) > 0.0 and ch.time_op(0, 0, reps=3) > 0.0
    with pytest.raises(_lib.NgsAMGError, match="Jacobi"):
        ch.time_op(0, 1)
    b = rhs(p, 2)                                              # the timing hook leaves a working handle behind
    lm = [ch.smoother_info(l)["lambda_max"] for l in range(H.n_levels - 1)] + [1.0]
    assert _rel(_mult(ch, b), ChebyRef(H, sm="cheby", lambda_max=lm).apply(b)) <= 1e-12


def test_rank_partitioned_hierarchies_refuse_the_type():
    import ctypes as C
    from ngsamg_amd import _lib
    from ngsamg_amd import dist as D
    comm = D.LoopbackComm(2)
    states = [D.assemble_poisson_owned(r, (2, 1, 1), (8, 8, 8)) for r in range(2)]
    with pytest.raises(_lib.NgsAMGError, match="cheby"):
        D.DistributedAMG(comm, states, dim=3, dist_min_rows=100, device=0, max_coarse_size=10, sm_type="cheby")
    # the C entry point itself: a descriptor whose levels ask for the type is refused before anything is built
    from ngsamg_amd.device import hierarchy_desc
    p, H = poisson_case((33, 33), "left|top", 5)
    top, keep1, _ = hierarchy_desc(H, sm_type="cheby", clev="none")
    tail, keep2, _ = hierarchy_desc(H, sm_type="jacobi")
    lib = _lib.hip()
    c = C.c_void_p()
    assert lib.amgx_comm_create(_lib.AMGX_COMM_LOCAL, 1, 0, None, 0, C.byref(c)) == 0
    try:
        dd = _lib.amgx_dist_desc()
        dd.top, dd.tail, dd.rank = top, tail, 0
        halo = (_lib.amgx_halo_desc * max(1, H.n_levels))()
        counts = np.array([H.levels[-1].n], dtype=np.int64)
        kmap = np.arange(H.levels[-1].n, dtype=np.int64)
        dd.halo, dd.counts, dd.kmap, dd.kmap_len = halo, _lib.ptr(counts, C.c_int64), _lib.ptr(kmap, C.c_int64), kmap.size
        out = C.c_void_p()
        assert lib.amgx_dist_create(c, C.byref(dd), C.byref(out)) != 0
        assert "Chebyshev" in lib.amgx_comm_last_error(c).decode(), lib.amgx_comm_last_error(c).decode()
    finally:
        lib.amgx_comm_destroy(c)


@pytest.mark.parametrize("cycle", ["V", "W"])
def test_mixed_hierarchy_cheby_and_gauss_seidel(cycle):
    """sm_type_spec = ["cheby", "gs"]: Chebyshev on level 0, multicolour Gauss-Seidel below; the reference takes the oracle's
    sweep in the device's colour order on the Gauss-Seidel levels"""
    from oracle.pyoracle import Oracle
    for name, (p, H) in (("poisson3d", poisson_case((17, 17, 17), "right|top", 20)), ("poisson2d", poisson_case((33, 33), "left|top", 5))):
        n = H.n_levels
        types = ["cheby"] + ["gs"] * (n - 1)
        lm = _lmax(H)
        orc = Oracle(H.levels, sm_type="gs_mc")

        def gs(l, x, b, res, ru, ur, xz, back):
            orc.smooth(l, x, b, res, ru, ur, xz, back)

        ref = ChebyRef(H, sm=["cheby"] + [gs] * (n - 1), degree=2, lambda_max=lm, cycle=cycle)
        b = rhs(p, 9)
        want = ref.apply(b)
        for env in (None, NO_DENSE):
            dev = _dev(H, env, sm_type=types, mg_cycle=cycle, cheb_lambda_max=lm)
            assert dev.smoother_info(0)["sm_type"] == "cheby" and dev.smoother_info(1)["sm_type"] == "gs"
            e = _rel(_mult(dev, b), want)
            print(name, cycle, e)
            assert e <= 1e-10, (name, cycle, e)                   # the project's Gauss-Seidel tolerance


def test_preconditioner_spec_mixes_the_types():
    from ngsamg_amd import NgsAMG, fem
    p = fem.poisson_fast((17, 17, 17), dirichlet="right|top")
    c = NgsAMG.h1_scal(to_matrix(p), p.free, ngs_amg_sm_type="gs", ngs_amg_sm_type_spec=["cheby"], ngs_amg_gs_hybrid=False)
    dev = c.GetAMGMatrix()._dev
    assert dev.smoother_info(0)["sm_type"] == "cheby" and dev.smoother_info(1)["sm_type"] == "gs"
    x = np.zeros(p.n)
    c.Mult(np.asarray(p.load, dtype=np.float64), x)
    assert np.isfinite(x).all() and np.linalg.norm(x) > 0


def test_standalone_smoother():
    from ngsamg_amd import NgsAMG, ngs_amg
    from ngsamg_amd.hierarchy import Level
    assert ngs_amg.CreateChebyshevSmoother is NgsAMG.CreateChebyshevSmoother
    p, H = poisson_case((33, 33), "left|top", 5)
    A = to_matrix(p)
    lv = H.levels[0]
    rng = np.random.default_rng(1)
    for degree, lam in ((2, None), (3, 1.9), (1, 2.5)):
        sm = NgsAMG.CreateChebyshevSmoother(A, p.free, degree=degree, ratio=8, lambda_max=lam)
        si = sm._amg._dev.smoother_info(0) if hasattr(sm, "_amg") else None
        one = Level(A=lv.A, P=None, PT=None, free=lv.free, dinv=lv.dinv, coords=None, color=lv.color, n_colors=lv.n_colors, agg=None)
        lmax = lam if lam is not None else 1.1 * power_estimate(one, 30)
        ref = ChebyRef([one, one], sm="cheby", degree=degree, ratio=8.0, lambda_max=[lmax, 1.0], clev="none")
        if si is not None:
            assert si["degree"] == degree and abs(si["lambda_max"] - lmax) <= 1e-10 * lmax and si["estimated"] == int(lam is None), si
        b = rng.standard_normal(p.n) * p.free
        x0 = rng.standard_normal(p.n) * p.free
        for back in (False, True):
            xr, rr = x0.copy(), np.zeros(p.n)
            ref.smooth(0, xr, b, rr, False, True, False, back)
            xg, rg = x0.copy(), np.zeros(p.n)
            (sm.SmoothBack if back else sm.Smooth)(xg, b, rg, False, True, False)
            assert _rel(xg, xr) <= 1e-12 and _rel(rg, rr) <= 1e-12, (degree, lam, back, _rel(xg, xr))
