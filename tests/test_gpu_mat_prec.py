"""Single-precision matrix storage for Chebyshev-smoothed levels (mat_prec = "single", AMGX_PREC_F32) on the device.

Definition under test: the smoother passes of a level that has the image (matrix_info(level, "A32")) read A rounded to float,
element by element; vectors, dinv, transfers, coarse inverse and the accumulation stay fp64, in the order of the fp64 kernels.
Hence a single-precision handle on H equals, BIT FOR BIT, a double handle on tests/mat_prec_ref.rounded_levels(H, levels that
report "A32") -- scalar and block levels alike (the block image keeps the layout and the order of additions of the fp64 one).

Every test first asserts that level 0 of its single-precision handle reports the image, so none can pass by running fp64.
cheb_lambda_max is passed explicitly to every handle of a comparison.

Tolerances: array_equal for the parity with the definition and for everything that stays fp64; 1e-12 relative against
the numpy reference (summation order); 1e-10 where a Gauss-Seidel level takes part; PCG iterations +-1, histories to rtol 1e-6."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.cheby_ref import ChebyRef, power_estimate
from tests.mat_prec_ref import RoundedHierarchy, pcg
from tests.problems import elasticity_case, poisson_case, rhs, to_matrix
from tests.test_mat_prec_cpu import problems

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
NO_FUSE = {"AMGX_CHEB_NO_FUSED_RESTRICT": "1"}
NO_F32 = {"AMGX_NO_MAT_F32": "1"}
ONE_LANE = {"AMGX_SELL_MAX_LANES": "1"}       # levels this small get several lanes per row; the big ones of a real run have one


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


@pytest.fixture(scope="module")
def lmax():
    """explicit per-level interval ends per problem, computed once (from the fp64 matrices, like the device's estimate)"""
    cache = {}

    def get(name, H):
        if name not in cache:
            cache[name] = [1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]] + [1.0]
        return cache[name]
    return get


def _image_levels(dev, H):
    """the levels whose smoother passes read the single-precision image; level 0 must be one of them"""
    fmts = [dev.matrix_info(l, "A32")["fmt"] for l in range(H.n_levels)]
    assert fmts[0] in ("sell", "bsell"), fmts
    assert fmts[-1] is None, fmts
    return [l for l, f in enumerate(fmts) if f is not None]


def _pair(H, lm, env=None, **kw):
    """(single-precision handle on H, double handle on the levels rounded where the first reports the image, those levels)"""
    single = _dev(H, env, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single", **kw)
    lv = _image_levels(single, H)
    double = _dev(RoundedHierarchy(H, lv), env, sm_type="cheby", cheb_lambda_max=lm, **kw)
    assert all(double.matrix_info(l, "A32")["fmt"] is None for l in range(H.n_levels))
    return single, double, lv


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


RUNS = ((False, True), (True, True), (True, False), (False, False))      # (device pointers, graph)


# ---- 3. bitwise parity with the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_bitwise_parity_with_the_rounded_double_handle(cycle, degree, lmax):
    seen = set()
    for name, (p, H), _ in problems():
        lm = lmax(name, H)
        b = rhs(p, 3)
        for env in ((None, NO_FUSE) if p.bs > 1 else (None, NO_FUSE, ONE_LANE)):
            single, double, lv = _pair(H, lm, env, mg_cycle=cycle, cheb_degree=degree)
            seen.add((single.matrix_info(0, "A32")["fmt"], H.levels[0].bs, single.matrix_info(0, "A32")["lanes"],
                      single.level_paths(0)["kernel"]))
            want = _mult(double, b)
            assert np.isfinite(want).all() and np.linalg.norm(want) > 0
            for device, graph in RUNS:
                got = _mult(single, b, device, graph)
                assert np.array_equal(got, want), (name, cycle, degree, env, device, graph, _rel(got, want))
            assert np.array_equal(_mult(double, b, True, False), want)
    print(sorted(seen, key=str))
    # scalar images with one and with several lanes per row, with and without the fused residual + restriction, and every block size
    assert {(f, bs) for f, bs, _, _ in seen} >= {("sell", 1), ("bsell", 3), ("bsell", 6)}, seen
    assert any(k == "cheby-res" for _, _, _, k in seen) and any(k is None for f, _, _, k in seen if f == "sell"), seen
    assert any(f == "sell" and g == 1 for f, _, g, _ in seen) and any(f == "sell" and g > 1 for f, _, g, _ in seen), seen


def test_bitwise_parity_two_by_two_blocks(lmax):
    """BSELL with 2x2 blocks: a 2-D elasticity hierarchy (displacements only)"""
    p, H = elasticity_case((21, 17), False, 5)
    assert H.levels[0].bs == 2
    lm = lmax("elasticity2d", H)
    b = rhs(p, 3)
    for degree in (1, 2, 3):
        single, double, lv = _pair(H, lm, cheb_degree=degree)
        assert single.matrix_info(0, "A32")["fmt"] == "bsell"
        want = _mult(double, b)
        for device, graph in RUNS:
            assert np.array_equal(_mult(single, b, device, graph), want), (degree, device, graph)


@pytest.mark.parametrize("steps,symm", [(2, False), (1, True), (2, True)])
def test_bitwise_parity_through_the_proxy_smoother(steps, symm, lmax):
    for name, case in (("poisson3d 17^3", poisson_case((17, 17, 17), "right|top", 20)),
                       ("elasticity 6x6/6x6", elasticity_case((13, 11, 9), True, 5, 0.12))):
        p, H = case
        lm = lmax(name, H)
        b = rhs(p, 6)
        for cycle in ("V", "W"):
            single, double, lv = _pair(H, lm, mg_cycle=cycle, sm_steps=steps, sm_symm=symm)
            want = _mult(double, b)
            for device, graph in RUNS:
                assert np.array_equal(_mult(single, b, device, graph), want), (name, cycle, steps, symm, device, graph)


# ---- 4. parity with the numpy reference on the rounded levels --------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
def test_cycle_matches_the_reference_on_rounded_levels(cycle, lmax):
    for name, (p, H), degrees in problems():
        lm = lmax(name, H)
        b = rhs(p, 3)
        for degree in degrees:
            for env in (None, NO_DENSE):
                single = _dev(H, env, sm_type="cheby", mg_cycle=cycle, cheb_degree=degree, cheb_lambda_max=lm, mat_prec="single")
                lv = _image_levels(single, H)
                ref = ChebyRef(RoundedHierarchy(H, lv), sm="cheby", degree=degree, lambda_max=lm, cycle=cycle).apply(b)
                for device, graph in RUNS[:2]:
                    e = _rel(_mult(single, b, device, graph), ref)
                    assert e <= 1e-12, (name, cycle, degree, env, device, graph, e)
                # the rounding is really there: the fp64 cycle is a different operator (how far it may move is bounded for the
                # V-cycle by tests/test_mat_prec_cpu.py; W and BS cycles smooth more often and move further, 1.0e-6 at most here)
                e64 = _rel(ChebyRef(H, sm="cheby", degree=degree, lambda_max=lm, cycle=cycle).apply(b), ref)
                assert e64 >= 1e-10, (name, cycle, degree, e64)


@pytest.mark.parametrize("steps,symm", [(1, False), (2, True)])
def test_smoother_flag_contract_on_the_image(steps, symm, lmax):
    import torch
    for name, case in (("poisson3d 17^3", poisson_case((17, 17, 17), "right|top", 20)),
                       ("elasticity 3x3/6x6", elasticity_case((13, 11, 9), False, 5, 0.12))):
        p, H = case
        lm = lmax(name, H)
        for degree in (1, 3):
            dev = _dev(H, sm_type="cheby", cheb_degree=degree, cheb_lambda_max=lm, sm_steps=steps, sm_symm=symm, mat_prec="single")
            lv = _image_levels(dev, H)
            RH = RoundedHierarchy(H, lv)
            ref = ChebyRef(RH, sm="cheby", degree=degree, lambda_max=lm, sm_steps=steps, sm_symm=symm)
            rng = np.random.default_rng(5)
            for l in range(min(2, H.n_levels - 1)):
                n = dev.sizes[l]
                A = RH.levels[l].A.to_scipy()
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
                                assert _rel(xg, xr) <= 1e-12, (name, l, back, ru, ur, xz, _rel(xg, xr))
                                if ur:
                                    assert _rel(rg, rr) <= 1e-12, (name, l, back, ru, ur, xz, _rel(rg, rr))
                                if l == 0 and not back:
                                    xd, bd, rd = (torch.from_numpy(v.copy()).cuda() for v in (x, b, res))
                                    dev.Smooth(l, xd, bd, rd, ru, ur, xz, back)
                                    torch.cuda.synchronize()
                                    assert np.array_equal(xd.cpu().numpy(), xg)
                                    if ur:
                                        assert np.array_equal(rd.cpu().numpy(), rg)


def test_update_res_reads_the_image(lmax):
    """update_res of amgx_smooth is a smoother pass: its residual is b - A32 x, not b - A x"""
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    lm = lmax("poisson3d 17^3", H)
    dev = _dev(H, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single")
    _image_levels(dev, H)
    A = H.levels[0].A.to_scipy()
    A32 = RoundedHierarchy(H, [0]).levels[0].A.to_scipy()
    b, x, res = rhs(p, 1), rhs(p, 2), np.zeros(p.n)
    dev.Smooth(0, x, b, res, False, True, False)
    r32, r64 = b - A32 @ x, b - A @ x
    assert _rel(res, r32) <= 1e-12, _rel(res, r32)
    assert _rel(r64, r32) >= 1e-10 and _rel(res, r64) >= 1e-10
    r = np.zeros(p.n)
    dev.Residual(0, x, b, r)                                              # amgx_residual keeps the fp64 image
    assert _rel(r, r64) <= 1e-13 and not np.array_equal(r, res)


def test_smooth_v_from_level_on_the_image(lmax):
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    lm = lmax("poisson3d 17^3", H)
    single, double, lv = _pair(H, lm)
    ref = ChebyRef(RoundedHierarchy(H, lv), sm="cheby", degree=2, lambda_max=lm)
    rng = np.random.default_rng(2)
    for l in range(H.n_levels - 1):
        n = single.sizes[l]
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
        xr, rr = x0.copy(), np.zeros(n)
        ref.smooth_v_from_level(l, xr, b, rr, False, True, False)
        xg, rg = x0.copy(), np.zeros(n)
        single.SmoothVFromLevel(l, xg, b, rg, False, True, False)
        assert _rel(xg, xr) <= 1e-12 and _rel(rg, rr) <= 1e-12, (l, _rel(xg, xr), _rel(rg, rr))
        xd, rd = x0.copy(), np.zeros(n)
        double.SmoothVFromLevel(l, xd, b, rd, False, True, False)
        assert np.array_equal(xg, xd) and np.array_equal(rg, rd), l


# ---- 5. what stays fp64 ----------------------------------------------------------------------------------------------------
def test_operator_queries_and_estimate_stay_double(lmax):
    for name, (p, H), _ in problems():
        single = _dev(H, sm_type="cheby", mat_prec="single")              # lambda_max estimated: on the fp64 image
        plain = _dev(H, sm_type="cheby")
        _image_levels(single, H)
        rng = np.random.default_rng(4)
        for l in range(H.n_levels):
            assert single.smoother_info(l) == plain.smoother_info(l), (name, l)
            n = single.sizes[l]
            x, b = rng.standard_normal(n), rng.standard_normal(n)
            ys, yp, rs, rp = (np.full(n, np.nan) for _ in range(4))
            single.MatVec(l, x, ys)
            plain.MatVec(l, x, yp)
            single.Residual(l, x, b, rs)
            plain.Residual(l, x, b, rp)
            assert np.array_equal(ys, yp) and np.array_equal(rs, rp), (name, l)
            assert _rel(ys, H.levels[l].A.to_scipy() @ x) <= 1e-13
        assert single.smoother_info(0)["estimated"] == 1
        X = np.ascontiguousarray(np.stack([rhs(p, 1), rhs(p, 2)]))
        Ys, Yp = np.full_like(X, np.nan), np.full_like(X, np.nan)
        single.MatVecMulti(0, X, Ys)
        plain.MatVecMulti(0, X, Yp)
        assert np.array_equal(Ys, Yp), name


def test_solve_converges_to_the_true_system(lmax):
    """A preconditioned solve to tol = 1e-12 ends with |b - A x| <= 1e-9 |b| on the free dofs for the UNROUNDED A.
    The bound separates the two candidates for the Krylov operator.  Measured on the CPU (the cycle of ChebyRef on the rounded
    levels, degree 2, tests/mat_prec_ref.pcg to 1e-12, over the 9 problems):
        fp64 operator:     2.2e-13 ... 1.3e-11   (a decade and more below 1e-9)
        rounded operator:  8.1e-8 ... 2.4e-6     (its true residual stalls near 2^-24 |A| |x| / |b|; a decade and more above)"""
    from ngsamg_amd.krylov import NativeCGSolver
    for name, (p, H), _ in problems():
        lm = lmax(name, H)
        dev = _dev(H, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single")
        _image_levels(dev, H)
        A = H.levels[0].A.to_scipy()
        free = np.repeat(np.asarray(p.free), p.bs).astype(bool)
        b = rhs(p, 3)
        cg = NativeCGSolver(dev, dev, tol=1e-12, maxsteps=100)
        x = np.asarray(cg.Solve(b))
        true_res = np.linalg.norm((b - A @ x)[free]) / np.linalg.norm(b)
        print(f"{name}: {cg.iterations} iterations, true residual {true_res:.2e}")
        assert cg.errors[-1] <= 1e-12 * cg.errors[0], (name, cg.iterations)
        assert true_res <= 1e-9, (name, true_res)


# ---- 6. PCG parity ---------------------------------------------------------------------------------------------------------
def test_pcg_parity(lmax):
    """iterations within +-1 of the double handle; histories against the reference cycle on the rounded levels inside the CG
    recurrence of ChebyRef.pcg WITH THE fp64 LEVEL-0 OPERATOR (tests/mat_prec_ref.pcg) -- what amgx_pcg is defined to run.
    (ChebyRef(rounded).pcg itself takes the rounded matrix as Krylov operator as well: another iteration, whose history differs
    from this one by 4e-7 ... 3e-4 on these problems.)"""
    from ngsamg_amd.krylov import NativeCGSolver
    for name, (p, H), degrees in problems():
        lm = lmax(name, H)
        b = rhs(p, 3)
        A = H.levels[0].A.to_scipy()
        for degree in degrees:
            single = _dev(H, sm_type="cheby", cheb_degree=degree, cheb_lambda_max=lm, mat_prec="single")
            plain = _dev(H, sm_type="cheby", cheb_degree=degree, cheb_lambda_max=lm)
            lv = _image_levels(single, H)
            its, errs = {}, {}
            for key, dev in (("single", single), ("double", plain)):
                cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
                cg.Solve(b)
                its[key], errs[key] = cg.iterations, np.asarray(cg.errors)
            ref = ChebyRef(RoundedHierarchy(H, lv), sm="cheby", degree=degree, lambda_max=lm)
            _, it_ref, errs_ref = pcg(ref, A, b, tol=1e-8, maxit=100)
            print(f"{name} degree {degree}: iterations single {its['single']} double {its['double']} reference {it_ref}")
            assert abs(its["single"] - its["double"]) <= 1, (name, degree, its)
            assert abs(its["single"] - it_ref) <= 1, (name, degree, its, it_ref)
            m = min(its["single"], it_ref) + 1
            assert np.allclose(errs["single"][:m], errs_ref[:m], rtol=1e-6, atol=0), (name, degree, errs["single"][:m], errs_ref[:m])


# ---- 7. edges --------------------------------------------------------------------------------------------------------------
def test_kill_switch_gives_the_double_handle(lmax):
    for name, case in (("poisson3d 17^3", poisson_case((17, 17, 17), "right|top", 20)),
                       ("elasticity 6x6/6x6", elasticity_case((13, 11, 9), True, 5, 0.12))):
        p, H = case
        lm = lmax(name, H)
        b = rhs(p, 3)
        on = _dev(H, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single")
        _image_levels(on, H)
        off = _dev(H, NO_F32, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single")
        plain = _dev(H, sm_type="cheby", cheb_lambda_max=lm)
        for l in range(H.n_levels):
            i = off.matrix_info(l, "A32")
            assert i["fmt"] is None and i["stream_bytes"] == 0 and i["stored"] == 0, (name, l, i)
        want = _mult(plain, b)
        for device, graph in RUNS:
            assert np.array_equal(_mult(off, b, device, graph), want), (name, device, graph)
        assert not np.array_equal(_mult(on, b), want)


@pytest.mark.parametrize("cycle", ["V", "W"])
def test_mixed_hierarchy_takes_the_image_on_its_chebyshev_levels(cycle, lmax):
    from oracle.pyoracle import Oracle
    for name, case in (("poisson3d 17^3", poisson_case((17, 17, 17), "right|top", 20)), ("poisson2d 33^2", poisson_case((33, 33), "left|top", 5))):
        p, H = case
        n = H.n_levels
        types = ["cheby"] + ["gs"] * (n - 1)
        lm = lmax(name, H)
        b = rhs(p, 9)
        for env in (None, NO_DENSE):
            dev = _dev(H, env, sm_type=types, mg_cycle=cycle, cheb_lambda_max=lm, mat_prec="single")
            assert _image_levels(dev, H) == [0]
            RH = RoundedHierarchy(H, [0])
            orc = Oracle(RH.levels, sm_type="gs_mc")

            def gs(l, x, bb, res, ru, ur, xz, back):
                orc.smooth(l, x, bb, res, ru, ur, xz, back)

            want = ChebyRef(RH, sm=["cheby"] + [gs] * (n - 1), degree=2, lambda_max=lm, cycle=cycle).apply(b)
            e = _rel(_mult(dev, b), want)
            assert e <= 1e-10, (name, cycle, env, e)                  # the project's Gauss-Seidel tolerance
        # per-level list: the same handle; "single" on the Gauss-Seidel level is refused before the library is called
        dev2 = _dev(H, sm_type=types, mg_cycle=cycle, cheb_lambda_max=lm, mat_prec=["single"] + ["double"] * (n - 1))
        assert np.array_equal(_mult(dev2, b), _mult(_dev(H, sm_type=types, mg_cycle=cycle, cheb_lambda_max=lm, mat_prec="single"), b))


def test_multi_vector_calls_stay_the_column_loop(lmax):
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    dev = _dev(H, sm_type="cheby", cheb_lambda_max=lmax("poisson3d 17^3", H), mat_prec="single")
    _image_levels(dev, H)
    B = np.ascontiguousarray(np.stack([rhs(p, j) for j in range(5)]))
    for k in (1, 2, 5):
        info = dev.multi_info(k)
        assert info["fused"] == 0 and info["groups"] == [1] * k, info
        X = np.full_like(B[:k], np.nan)
        dev.MultMulti(np.ascontiguousarray(B[:k]), X)
        for j in range(k):
            assert np.array_equal(X[j], _mult(dev, np.ascontiguousarray(B[j]))), (k, j)


def test_values_beyond_single_precision_are_refused():
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import Matrix
    p, H = poisson_case((17, 17, 17), "right|top", 20)
    A = H.levels[0].A
    val = np.array(A.val, dtype=np.float64)
    val[7] = 1e39
    bad = RoundedHierarchy(H, [])
    import dataclasses
    bad.levels[0] = dataclasses.replace(H.levels[0], A=Matrix(A.n_rows, A.n_cols, A.br, A.bc, A.rowptr, A.col, val))
    with pytest.raises(_lib.NgsAMGError, match="single precision") as ei:
        _dev(bad, sm_type="cheby", cheb_lambda_max=2.5, mat_prec="single")
    assert "level 0" in str(ei.value)
    _dev(bad, sm_type="cheby", cheb_lambda_max=2.5)                       # the double handle takes the matrix


def test_c_abi_refuses_bad_requests():
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = poisson_case((33, 33), "left|top", 5)
    lib = _lib.hip()
    for sm, level, value, msgs in (("cheby", 0, 2, ("mat_prec", "level 0")), ("cheby", 1, -1, ("mat_prec", "level 1")),
                                   ("jacobi", 0, 1, ("level 0", "Chebyshev")), (["cheby", "gs"] + ["cheby"] * (H.n_levels - 2), 1, 1, ("level 1", "Chebyshev"))):
        desc, keep, _ = hierarchy_desc(H, sm_type=sm)
        desc.levels[level].mat_prec = value
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, (sm, level, value)
        msg = lib.amgx_last_error(None).decode()
        assert all(m in msg for m in msgs), msg
    # the coarsest level ignores the field
    desc, keep, _ = hierarchy_desc(H, sm_type="cheby")
    desc.levels[H.n_levels - 1].mat_prec = 1
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) == 0, lib.amgx_last_error(None).decode()
    lib.amgx_destroy(h)
    # the queries: which = 7 is the last one
    dev = _dev(H, sm_type="cheby", mat_prec="single")
    fmt, stored, lanes, nb = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
    assert lib.amgx_matrix_info(dev._h, 0, 7, C.byref(fmt), C.byref(stored), C.byref(lanes)) == 0 and fmt.value in (1, 2)
    assert lib.amgx_matrix_info(dev._h, 0, 8, C.byref(fmt), C.byref(stored), C.byref(lanes)) != 0
    assert "0..7" in lib.amgx_last_error(dev._h).decode()
    assert lib.amgx_matrix_stream_bytes(dev._h, 0, 8, C.byref(nb)) != 0 and lib.amgx_matrix_stream_bytes(dev._h, 0, -1, C.byref(nb)) != 0


def test_stream_bytes_of_the_image():
    for name, (p, H), _ in problems():
        dev = _dev(H, sm_type="cheby", mat_prec="single")
        for l in _image_levels(dev, H):
            a, a32 = dev.matrix_info(l, "A"), dev.matrix_info(l, "A32")
            assert a32["fmt"] == a["fmt"] and a32["lanes"] == a["lanes"] and a32["stored"] == a["stored"], (name, l, a, a32)
            bs = H.levels[l].bs
            # stored values: every stored entry of a sliced-ELL image; a block step of BSELL holds bs values in each of 64 lanes
            values = a["stored"] if bs == 1 else (a["stored"] // (64 // bs)) * bs * 64
            assert 0 < a32["stream_bytes"] < a["stream_bytes"], (name, l)
            assert a["stream_bytes"] - a32["stream_bytes"] == 4 * values, (name, l, a, a32, values)


def test_time_ops_and_standalone_smoother(lmax):
    from ngsamg_amd import NgsAMG
    p, H = poisson_case((33, 33), "left|top", 5)
    lm = lmax("poisson2d 33^2", H)
    dev = _dev(H, sm_type="cheby", cheb_lambda_max=lm, mat_prec="single")
    lv = _image_levels(dev, H)
    assert dev.time_op(0, 10, reps=3) > 0.0 and dev.time_op(0, 5, reps=3) > 0.0 and dev.time_op(0, 0, reps=3) > 0.0
    b = rhs(p, 2)                                                         # the timing hooks leave a working handle behind
    assert _rel(_mult(dev, b), ChebyRef(RoundedHierarchy(H, lv), sm="cheby", lambda_max=lm).apply(b)) <= 1e-12
    # the stand-alone smoother: one level, which is smoothed and takes the image
    A = to_matrix(p)
    rng = np.random.default_rng(1)
    x0, bb = rng.standard_normal(p.n) * p.free, rng.standard_normal(p.n) * p.free
    out = {}
    for prec in ("double", "single"):
        sm = NgsAMG.CreateChebyshevSmoother(A, p.free, degree=3, lambda_max=2.2, mat_prec=prec)
        x, r = x0.copy(), np.zeros(p.n)
        sm.Smooth(x, bb, r, False, True, False)
        out[prec] = x
    e = _rel(out["single"], out["double"])
    assert 1e-10 <= e <= 1e-6, e
