"""AMGX_MULTI_FUSE (fuse=True): fused multi-vector cycles on Chebyshev and block levels.

References: tests.cheby_ref.ChebyRef (Chebyshev and mixed hierarchies), oracle.pyoracle.Oracle (block Jacobi),
tests.mat_prec_ref.RoundedHierarchy (single-precision image), scipy (level products).  Tolerances are the project's
(DESIGN.md 3): order-free cycles 1e-12 relative, products and same-arithmetic comparisons 1e-13, PCG iterations +-1,
histories rtol 1e-6, residuals 1e-8.  Every handle of a comparison gets an explicit cheb_lambda_max."""
import functools
import os

import numpy as np
import pytest

from tests.cheby_ref import ChebyRef, power_estimate
from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
NO_RB = {"AMGX_NO_RB_TRANSFER": "1"}          # keeps the transfers of the elasticity hierarchies in the general block-CSR form
NO_BSELL = {"AMGX_NO_BSELL": "1"}             # keeps the block level matrices in block CSR
ONE_LANE = {"AMGX_SELL_MAX_LANES": "1"}       # one lane per row also where the rows are long (A of the Chebyshev levels)


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


@functools.lru_cache(maxsize=None)
def _case(name):
    return {"poisson 17^3": lambda: poisson_case((17, 17, 17), "right|top", 20),
            "poisson 25^3": lambda: poisson_case((25, 25, 25), "right|top", 20),
            "elast 9x8x7": lambda: elasticity_case((9, 8, 7), False, 5, 0.12),            # 504 block rows: 24 slices of 3x3, 50.4 of 6x6
            "elast 9x8x7 rot": lambda: elasticity_case((9, 8, 7), True, 5, 0.12),
            "elast 13x11x9": lambda: elasticity_case((13, 11, 9), False, 5, 0.12),        # 1287 block rows: last slice partly idle
            "elast 13x11x9 rot": lambda: elasticity_case((13, 11, 9), True, 5, 0.12),
            "elast2d 21x17": lambda: elasticity_case((21, 17), False, 5),                 # 2x2 blocks, 357 block rows, 32 per slice
            "elast2d 21x17 rot": lambda: elasticity_case((21, 17), True, 5)}[name]()


CASES = ["poisson 17^3", "poisson 25^3", "elast 9x8x7", "elast 9x8x7 rot", "elast 13x11x9", "elast 13x11x9 rot", "elast2d 21x17",
         "elast2d 21x17 rot"]
ELAST = [c for c in CASES if c.startswith("elast")]


@functools.lru_cache(maxsize=None)
def _lmax(name):
    H = _case(name)[1]
    return tuple(1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]) + (1.0,)


def _mixed(H):
    return [("jacobi", "cheby")[l % 2] for l in range(H.n_levels)]


# a handle specification: (case, kind, degree, extra environment); kind: "cheby", "jacobi" (block Jacobi) or "mixed"
SPECS = ([(c, "cheby", d, None) for c in CASES for d in (1, 2, 3, 4)]
         + [(c, "jacobi", 0, None) for c in ("elast 9x8x7", "elast 13x11x9 rot", "elast2d 21x17")]
         + [(c, "mixed", 2, None) for c in ("poisson 25^3", "elast 13x11x9", "elast 13x11x9 rot")]
         + [("elast 9x8x7", "cheby", 2, "no_rb"), ("elast 13x11x9 rot", "cheby", 3, "no_rb"), ("elast2d 21x17", "cheby", 2, "no_rb"),
            ("elast 13x11x9", "cheby", 2, "no_bsell"), ("elast 9x8x7 rot", "jacobi", 0, "no_bsell"),
            ("poisson 25^3", "cheby", 3, "one_lane")])
EXTRA = {None: {}, "no_rb": NO_RB, "no_bsell": NO_BSELL, "one_lane": ONE_LANE}


def _spec_id(s):
    return f"{s[0]}-{s[1]}{s[2] or ''}" + (f"-{s[3]}" if s[3] else "")


def _handle(spec, env=None, **more):
    name, kind, degree, extra = spec
    H = _case(name)[1]
    kw = dict(more)
    if kind == "jacobi":
        kw.update(sm_type="jacobi")
    else:
        kw.update(sm_type="cheby" if kind == "cheby" else _mixed(H), cheb_degree=degree, cheb_lambda_max=list(_lmax(name)))
    return _dev(H, dict(env or {}, **EXTRA[extra]), **kw)


@functools.lru_cache(maxsize=None)
def _block(name, k=8, seed=0):
    p = _case(name)[0]
    B = np.stack([rhs(p, seed + j) for j in range(k)])
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def _reference(name, kind, degree):
    """the cycle of a specification on the 8 columns of _block(name), computed once"""
    H = _case(name)[1]
    if kind == "jacobi":
        from oracle.pyoracle import Oracle
        ref = Oracle(H.levels, sm_type="jacobi")
    else:
        ref = ChebyRef(H, sm="cheby" if kind == "cheby" else _mixed(H), degree=degree, lambda_max=list(_lmax(name)))
    X = np.stack([ref.apply(np.array(b)) for b in _block(name)])
    X.setflags(write=False)
    return X


def _mult(dev, B, interleaved=False, device=False, graph=True, fuse=True):
    """X = C B through MultMulti; B and the result are (k, n) whatever the layout handed to the library"""
    Bin = np.array(B.T if interleaved else B, order="C")            # (a writable copy: the shared blocks are read-only)
    if device:
        import torch
        Bd = torch.from_numpy(Bin).cuda()
        Xd = torch.full_like(Bd, float("nan"))
        dev.MultMulti(Bd, Xd, interleaved=interleaved, graph=graph, fuse=fuse)
        torch.cuda.synchronize()
        X = Xd.cpu().numpy()
    else:
        X = np.full_like(Bin, np.nan)
        dev.MultMulti(Bin, X, interleaved=interleaved, graph=graph, fuse=fuse)
    return np.ascontiguousarray(X.T) if interleaved else X


def _single(dev, B):
    X = np.empty_like(B)
    for j in range(B.shape[0]):
        dev.Mult(np.ascontiguousarray(B[j]), X[j])
    return X


def _check_plan(dev, k, plan):
    assert plan["fused"] == 1 and plan["note"] == "", (k, plan)
    assert sum(plan["groups"]) == k and set(plan["groups"]) <= {1, 2, 4}, (k, plan)
    if k == 4:
        assert max(plan["groups"]) >= 2, plan
    assert plan["work_bytes"] > 0 or k == 1, (k, plan)


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------
PLAN_SPECS = [("poisson 17^3", "cheby", 2, None), ("elast 9x8x7", "cheby", 2, None), ("elast 9x8x7 rot", "cheby", 1, None),
              ("elast 9x8x7", "jacobi", 0, None), ("elast 9x8x7 rot", "jacobi", 0, None), ("poisson 17^3", "mixed", 2, None)]


@pytest.mark.parametrize("spec", PLAN_SPECS, ids=_spec_id)
def test_plan_of_qualifying_handles(spec):
    dev = _handle(spec)
    for k in range(1, 9):
        _check_plan(dev, k, dev.multi_plan(k, fuse=True))
        # (amgx_multi_info forwards to amgx_multi_plan with flags = 0, so this equality holds by construction; that multi_info
        # answers as before is what the next line and the untouched tests of test_gpu_multi_rhs.py / test_gpu_cheby.py check)
        off, info = dev.multi_plan(k, fuse=False), dev.multi_info(k)
        assert {key: off[key] for key in info} == info, (k, off, info)
        assert info["fused"] == 0 and info["groups"] == [1] * k and off["note"] != "", (k, off)     # none of them is scalar Jacobi
    # a Chebyshev level costs one more vector than a Jacobi level of the same hierarchy
    if spec[1] == "cheby" and spec[0].startswith("elast"):
        che, jac = _handle(spec, NO_DENSE), _handle((spec[0], "jacobi", 0, None), NO_DENSE)
        assert che.multi_plan(4, fuse=True)["work_bytes"] > jac.multi_plan(4, fuse=True)["work_bytes"]


def test_plan_of_a_scalar_jacobi_handle_is_fused_either_way():
    p, H = _case("poisson 17^3")
    dev = _dev(H, sm_type="jacobi")
    for k in range(1, 9):
        on, off, info = dev.multi_plan(k, fuse=True), dev.multi_plan(k, fuse=False), dev.multi_info(k)
        assert {key: off[key] for key in info} == info and info["fused"] == 1
        assert on == off and on["note"] == "", (on, off)
    B = np.array(_block("poisson 17^3")[:4])
    assert np.array_equal(_mult(dev, B, device=True, fuse=True), _mult(dev, B, device=True, fuse=False))     # one path, with or without


@pytest.mark.parametrize("which", ["gs", "hgs", "W", "BS", "steps2"])
def test_plan_of_handles_that_keep_the_column_loop(which):
    from ngsamg_amd import fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    p, H = _case("poisson 17^3")
    lm = list(_lmax("poisson 17^3"))
    if which in ("gs", "hgs"):
        ps = fem.poisson_fast((21, 21, 21))                   # the problem of smoke()
        H = Hierarchy(Matrix(ps.n, ps.n, 1, 1, ps.rowptr, ps.col, ps.val), ps.free, ps.coords, dim=3, energy=0, max_coarse_size=20)
        dev, word = _dev(H, sm_type=which), "smoother"
    elif which in ("W", "BS"):
        dev, word = _dev(H, sm_type="cheby", mg_cycle=which, cheb_lambda_max=lm), "cycle"
    else:
        dev, word = _dev(H, sm_type="cheby", sm_steps=2, cheb_lambda_max=lm), "sm_steps"
    for k in (1, 3, 4, 8):
        plan = dev.multi_plan(k, fuse=True)
        assert plan["fused"] == 0 and plan["groups"] == [1] * k, plan
        assert word in plan["note"], plan
        if word != "cycle":
            assert "level 0" in plan["note"], plan
    B = np.stack([rhs(p if which not in ("gs", "hgs") else ps, j) for j in range(3)])
    assert np.array_equal(_mult(dev, B, fuse=True), _single(dev, B))       # the flag is never an error


# ---- 2. the fused cycle against the reference -------------------------------------------------------------------------------
def _uses_chunk_local_restriction(dev):
    return any(dev.level_paths(l)["kernel"] is not None for l in range(dev.n_levels))


@pytest.mark.parametrize("spec", SPECS, ids=_spec_id)
def test_fused_cycle_matches_reference(spec):
    name, kind, degree, extra = spec
    B, ref = _block(name), _reference(name, kind, degree)
    for env in (None, NO_DENSE):
        dev = _handle(spec, env)
        ci = dev.cycle_info()
        assert (ci["dense_level"] < 0) == (env is NO_DENSE), ci
        worst = 0.0
        for k in range(1, 9):
            _check_plan(dev, k, dev.multi_plan(k, fuse=True))
            for interleaved in (False, True):
                for device in (False, True):
                    for graph in (True, False):
                        X = _mult(dev, B[:k], interleaved, device, graph)
                        for j in range(k):
                            e = _rel(X[j], ref[j])
                            worst = max(worst, e)
                            assert e <= 1e-12, (spec, env, k, interleaved, device, graph, j, e)
        # against the single-vector path of the same handle: 1e-13 where both run the literal cycle kernel by kernel; 1e-12 where
        # the single-vector down pass is the chunk-local fused residual + restriction (another summation order in P^T r)
        tol = 1e-12 if _uses_chunk_local_restriction(dev) else 1e-13
        one = _single(dev, np.array(B))
        em = 0.0
        for k, interleaved, device in ((8, False, False), (2, True, True), (7, False, True), (4, True, False)):   # 4 + 4, 2, 4 + 2 + 1, 4
            X = _mult(dev, B[:k], interleaved, device)
            em = max(em, max(_rel(X[j], one[j]) for j in range(k)))
            if k == 7:
                assert np.array_equal(X[6], one[6]), (spec, env)      # the single column IS the single-vector path
        print(f"{_spec_id(spec)} dense={ci['dense_level']}: vs reference {worst:.2e}, vs Mult {em:.2e} (bound {tol:.0e})")
        assert em <= tol, (spec, env, em, tol)


# ---- 3. every kernel family is exercised by the handles of (2) --------------------------------------------------------------
def test_coverage_of_formats_and_shapes():
    seen = set()
    for spec in sorted({(s[0], s[1], 2 if s[1] != "jacobi" else 0, s[3]) for s in SPECS}, key=str):
        p, H = _case(spec[0])
        dev = _handle(spec, NO_DENSE)
        assert dev.cycle_info()["dense_level"] < 0
        for l in range(H.n_levels - 1):                       # the levels the multi cycle runs level by level
            lv = H.levels[l]
            mi = dev.matrix_info(l, "A")
            if lv.A.br == 1:
                assert mi["fmt"] in ("sell", "sellwin", "csrvec"), (spec, l, mi)
                seen.add(("A", mi["fmt"], "1" if mi["lanes"] == 1 else ">1") if mi["fmt"] == "sell" else ("A", mi["fmt"]))
            else:
                assert mi["fmt"] in ("bsell", "csrvec"), (spec, l, mi)
                seen.add(("A", "bsell" if mi["fmt"] == "bsell" else "bcsr", lv.A.br))
            for which, M in (("P", lv.P), ("PT", lv.PT)):
                mi = dev.matrix_info(l, which)
                if M.br == 1 and M.bc == 1:
                    assert mi["fmt"] in ("sell", "sellwin", "csrvec"), (spec, l, which, mi)
                    seen.add(("T", mi["fmt"], "1" if mi["lanes"] == 1 else ">1") if mi["fmt"] == "sell" else ("T", mi["fmt"]))
                elif mi["fmt"] == "rigid-body":
                    seen.add(("T", "rb", lv.P.br, lv.P.bc, 2 if "2d" in spec[0] else 3))
                else:
                    assert mi["fmt"] == "csrvec", (spec, l, which, mi)
                    seen.add(("T", "bcsr", M.br, M.bc))
    print(sorted(seen, key=str))
    # A (the EP_CHEB / EP_RES / EP_JAC kernels): SELL with one lane (AMGX_SELL_MAX_LANES=1 handle) and with several, CSR-vector,
    # BSELL 2 / 3 / 6, block CSR.  A level matrix is never stored as windowed SELL: amgx_create asks for length-sorted windows for the
    # transfers only (upload_matrix is called with win = 0 for A, and no switch changes that), so the windowed kernel is reached
    # through P / P^T (EP_AXPY / EP_MULT), which is asserted instead.
    want = {("A", "sell", "1"), ("A", "sell", ">1"), ("A", "csrvec"), ("T", "sellwin"), ("A", "bsell", 2), ("A", "bsell", 3),
            ("A", "bsell", 6), ("T", "rb", 6, 6, 3), ("T", "rb", 3, 6, 3)}
    assert want <= seen, want - seen
    assert ("A", "sellwin") not in seen, seen
    assert any(s[:2] == ("T", "sell") for s in seen), seen
    assert any(s[:2] == ("A", "bcsr") for s in seen), seen
    assert any(s[:2] == ("T", "rb") and s[4] == 2 for s in seen), seen
    assert any(s[:2] == ("T", "bcsr") for s in seen), seen       # (AMGX_NO_RB_TRANSFER keeps the general form)


# ---- 4. no cross-talk between the columns -----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [("poisson 25^3", "cheby", 2, None), ("elast 13x11x9 rot", "cheby", 2, None)], ids=_spec_id)
@pytest.mark.parametrize("env", [None, NO_DENSE], ids=["default", "no_dense_tail"])
def test_columns_do_not_talk_to_each_other(spec, env):
    p = _case(spec[0])[0]
    dev = _handle(spec, env)
    free = np.repeat(p.free, p.bs).astype(bool)
    rng = np.random.default_rng(5)
    B8 = np.array(_block(spec[0], seed=20))
    X8 = _mult(dev, B8)
    for k in (2, 4, 8):
        B = B8[:k]
        X = _mult(dev, B)
        perm = rng.permutation(k)
        while np.array_equal(perm, np.arange(k)):
            perm = rng.permutation(k)
        assert np.array_equal(_mult(dev, B[perm]), X[perm]), k
        assert np.array_equal(_mult(dev, B[perm], interleaved=True, device=True), X[perm]), k
        Bn = B.copy()
        Bn[k // 2] = np.nan
        Xn = _mult(dev, Bn)
        keep = [j for j in range(k) if j != k // 2]
        assert np.array_equal(Xn[keep], X[keep]), k
        assert np.all(np.isnan(Xn[k // 2][free])), k
        for j in range(k):
            e = _rel(X[j], X8[j])
            assert e <= 1e-13, (k, j, e)
    # k = 1 with the flag is the single-vector path itself; so is the single column of k = 7 = 4 + 2 + 1
    assert np.array_equal(_mult(dev, B8[:1]), _single(dev, B8[:1]))
    assert np.array_equal(_mult(dev, B8[:1], interleaved=True, device=True), _single(dev, B8[:1]))
    X7 = _mult(dev, B8[:7])
    assert np.array_equal(X7[6], _single(dev, B8[6:7])[0])
    assert np.array_equal(X7[:4], _mult(dev, B8[:4]))


# ---- 5. the single-precision image ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poisson 17^3", "elast 13x11x9"])
def test_single_precision_image(name):
    from tests.mat_prec_ref import RoundedHierarchy
    p, H = _case(name)
    lm = list(_lmax(name))
    B = np.array(_block(name))
    for env in (None, NO_DENSE):
        dev = _dev(H, env, sm_type="cheby", cheb_degree=2, cheb_lambda_max=lm, mat_prec="single")
        assert dev.matrix_info(0, "A32")["fmt"] is not None
        with32 = [l for l in range(H.n_levels - 1) if dev.matrix_info(l, "A32")["fmt"] is not None]
        assert dev.multi_plan(4, fuse=True)["fused"] == 1
        ref32 = ChebyRef(RoundedHierarchy(H, with32), sm="cheby", degree=2, lambda_max=lm)
        ref64 = ChebyRef(H, sm="cheby", degree=2, lambda_max=lm)
        for k in (2, 4, 7):
            X = _mult(dev, B[:k], interleaved=(k == 4), device=(k != 2))
            for j in range(k if k != 7 else 6):               # (the seventh column of 4 + 2 + 1 is amgx_apply itself)
                e32, e64 = _rel(X[j], ref32.apply(B[j])), _rel(X[j], ref64.apply(B[j]))
                print(f"{name} k={k} column {j}: rounded reference {e32:.2e}, fp64 reference {e64:.2e}")
                assert e32 <= 1e-12, (name, k, j, e32)
                assert e64 >= 1e-10, (name, k, j, e64)      # the rounding is real
        # the level product stays fp64
        A = H.levels[0].A.to_scipy()
        Y = np.full_like(B[:4], np.nan)
        dev.MatVecMulti(0, np.ascontiguousarray(B[:4]), Y, fuse=True)
        for j in range(4):
            assert _rel(Y[j], A @ B[j]) <= 1e-13, (name, j)


# ---- 6. level products ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [("poisson 25^3", "cheby", 2, None), ("elast 13x11x9", "cheby", 2, None),
                                  ("elast 13x11x9", "cheby", 2, "no_bsell")], ids=_spec_id)
def test_level_products(spec):
    import torch
    H = _case(spec[0])[1]
    dev = _handle(spec)
    rng = np.random.default_rng(7)
    for l in range(dev.n_levels):
        A = H.levels[l].A.to_scipy()
        X = rng.standard_normal((8, dev.sizes[l]))
        ref = np.stack([A @ x for x in X])
        for k in range(1, 9):
            for interleaved in (False, True):
                Xin = np.ascontiguousarray(X[:k].T) if interleaved else np.ascontiguousarray(X[:k])
                Y = np.full_like(Xin, np.nan)
                dev.MatVecMulti(l, Xin, Y, interleaved=interleaved, fuse=True)
                Yd = torch.full(Xin.shape, float("nan"), dtype=torch.float64, device="cuda")
                dev.MatVecMulti(l, torch.from_numpy(Xin).cuda(), Yd, interleaved=interleaved, fuse=True)
                torch.cuda.synchronize()
                assert np.array_equal(Yd.cpu().numpy(), Y), (l, k, interleaved)
                Y = Y.T if interleaved else Y
                for j in range(k):
                    assert _rel(Y[j], ref[j]) <= 1e-13, (l, k, interleaved, j, _rel(Y[j], ref[j]))


# ---- 7. graphs are keyed by k, the layout and the flag ----------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("spec", [("poisson 17^3", "cheby", 2, None), ("elast 9x8x7", "cheby", 3, None)], ids=_spec_id)
def test_graph_replay_with_changing_k_and_flag_on_the_same_buffers(spec, device):
    import torch
    p = _case(spec[0])[0]
    dev = _handle(spec, NO_DENSE)
    n = dev.sizes[0]
    B = np.array(_block(spec[0])[:4])
    ref = _reference(*spec[:3])
    loop = _single(dev, B)
    stream = torch.cuda.Stream() if device else None          # (the legacy default stream cannot be captured)
    if device:
        bbuf = torch.from_numpy(B.reshape(-1).copy()).cuda()
        xbuf = torch.empty_like(bbuf)
    else:
        bbuf, xbuf = B.reshape(-1).copy(), np.empty(4 * n)

    def run(k, interleaved, fuse, graph=True):
        src = B[:k].T if interleaved else B[:k]
        shape = (n, k) if interleaved else (k, n)
        if device:
            bbuf[: k * n].copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
            xbuf.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                dev.MultMulti(bbuf[: k * n].view(shape), xbuf[: k * n].view(shape), interleaved=interleaved, graph=graph, fuse=fuse)
            torch.cuda.synchronize()
            X = xbuf[: k * n].view(shape).cpu().numpy()
        else:
            bbuf[: k * n] = np.ascontiguousarray(src).reshape(-1)
            xbuf[:] = np.nan
            X = xbuf[: k * n].reshape(shape)
            dev.MultMulti(bbuf[: k * n].reshape(shape), X, interleaved=interleaved, graph=graph, fuse=fuse)
            X = X.copy()
        return np.ascontiguousarray(X.T) if interleaved else X

    got = {}
    steps = [(4, False, True), (2, False, True), (4, False, False), (4, False, True), (4, True, True), (2, True, False), (2, True, True),
             (4, False, False), (3, False, True), (4, True, True), (3, False, False)]
    for step, (k, il, fuse) in enumerate(steps):
        X = run(k, il, fuse)
        if fuse:
            for j in range(k):
                assert _rel(X[j], ref[j]) <= 1e-12, (step, k, il, j)
        else:
            assert np.array_equal(X, loop[:k]), (step, k, il)                  # without the flag: the column loop, bit for bit
        if (k, il, fuse) in got:
            assert np.array_equal(X, got[(k, il, fuse)]), (step, k, il, fuse)  # the replay
        got[(k, il, fuse)] = X
    for (k, il, fuse), X in got.items():
        assert np.array_equal(run(k, il, fuse, graph=False), X), (k, il, fuse)   # direct launches


# ---- 8. k independent CG recurrences ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["elasticity rotations, degree 1", "poisson 25^3, degree 2"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_solve_multi(which, device):
    import torch
    from ngsamg_amd.krylov import NativeCGSolver
    if which.startswith("elast"):
        p, H = elasticity_case((10, 10, 10), True, 20)            # the rotations problem of tests/test_cheby_cpu.py's budget table
        degree = 1
    else:
        p, H = _case("poisson 25^3")
        degree = 2
    lm = [1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]] + [1.0]
    dev = _dev(H, sm_type="cheby", cheb_degree=degree, cheb_lambda_max=lm)
    assert dev.multi_plan(4, fuse=True)["fused"] == 1 and dev.multi_plan(4, fuse=True)["groups"] == [4]
    n = dev.sizes[0]
    free = np.repeat(p.free, p.bs).astype(np.float64)
    rng = np.random.default_rng(0)
    B = np.stack([np.asarray(p.load, dtype=np.float64).reshape(-1) * free, rng.standard_normal(n) * free, rng.standard_normal(n) * free,
                  np.zeros(n)])
    interleaved = device
    lay = (lambda M: np.ascontiguousarray(M.T)) if interleaved else np.ascontiguousarray
    tol = 1e-10
    cg = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
    if device:
        sol = torch.from_numpy(lay(np.zeros_like(B))).cuda()
        cg.SolveMulti(torch.from_numpy(lay(B)).cuda(), sol, interleaved=interleaved, fuse=True)
        torch.cuda.synchronize()
        X = sol.cpu().numpy()
    else:
        X = lay(np.zeros_like(B))
        cg.SolveMulti(lay(B), X, interleaved=interleaved, fuse=True)
    X = X.T if interleaved else X
    its, errs = cg.iterations, cg.errors
    assert its[3] == 0 and errs[3] == [0.0] and not X[3].any() and not np.signbit(X[3]).any()
    A = H.levels[0].A.to_scipy()
    f = free.astype(bool)
    for j in range(3):
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        to_1e8 = next(i for i, e in enumerate(errs[j]) if e <= 1e-8 * errs[j][0])
        print(f"{which} column {j}: iterations multi {its[j]} single {one.iterations}; to 1e-8: {to_1e8}")
        assert abs(its[j] - one.iterations) <= 1, (j, its[j], one.iterations)
        assert len(errs[j]) == its[j] + 1
        m = min(its[j], one.iterations)
        assert np.allclose(errs[j][:m], one.errors[:m], rtol=1e-6, atol=0), j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j
        if which.startswith("elast") and j == 0:
            assert to_1e8 <= 20, to_1e8                           # degree 1 on the rotations problem: the budget of the design table
