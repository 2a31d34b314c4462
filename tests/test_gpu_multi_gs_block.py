"""AMGX_MULTI_FUSE_GS_BLOCK (fuse="gs_block"): fused multi-vector cycles with Gauss-Seidel on 2x2 / 3x3 / 6x6 levels in
the hybrid-block, the block-coloured and the two block multicolour forms.

References: the single-vector sweep of the same handle (bit for bit, through SmoothMulti / Smooth), oracle.pyoracle.Oracle with
tests.hgs_oracle.hgs_levels for hgs and sm_type="gs_mc" for gs (the project's bound for Gauss-Seidel in the GPU's order: 1e-10
relative), Mult of the same handle (1e-12, the bound of DESIGN.md 5.13 / 5.15).  PCG: iterations +-1, histories rtol 1e-6, true
residuals 1e-8.  The mixed handle (hgs on level 0, Chebyshev below) has no oracle of its own and is held against Mult only.

Measured maxima on an MI355X (the prints of test_cycle_matches_oracle_and_mult): see DESIGN.md 5.16."""
import functools
import os

import numpy as np
import pytest

from tests.problems import elasticity_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
BC = {"AMGX_BGSB_BC_MIN_ROWS": "0"}
NO_SPLIT = {"AMGX_BGSB_NO_SPLIT": "1"}
BSELL = {"AMGX_BGS_BSELL_MIN": "1"}
FUSE = "gs_block"
BLOCK_FORMS = {"hybrid-block", "block-coloured", "mc-block-rowlist", "mc-block-bsell"}

# shape -> (grid, rotations, block size of level 0, block rows of level 0, gs_block_rows of level 0).  Partial last sweep blocks:
# 2184 = 34 * 63 + 42 and 1440 = 22 * 64 + 32 on level 0, 263 = 4 * 60 + 23 on level 1 of "3d"; 1320 = 22 * 60 has none (the partial
# 6x6 sweep block is the one of "3d" level 1)
SHAPES = {"3d": ((14, 13, 12), False, 3, 2184, 63), "rot": ((12, 11, 10), True, 6, 1320, 60), "2d": ((40, 36), False, 2, 1440, 64)}


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


# handle specifications: name -> (shape, smoother, environment)
SPECS = {
    "3d-hgs": ("3d", "hgs", {}),                                   # dense tail: only level 0 sweeps
    "3d-hgs-levels": ("3d", "hgs", NO_DENSE),                      # level 1 hybrid-block (263 rows of 6x6), multicolour block forms below
    "3d-hgs-nosplit": ("3d", "hgs", NO_SPLIT),                     # the sweep from zero, then EP_RES on A
    "3d-hgs-nosplit-levels": ("3d", "hgs", _env(NO_SPLIT, NO_DENSE)),
    "3d-bc": ("3d", "hgs", BC),                                    # one in-place launch per block colour
    "3d-bc-levels": ("3d", "hgs", _env(BC, NO_DENSE)),
    "3d-bc-nosplit": ("3d", "hgs", _env(BC, NO_SPLIT)),            # zeroes x and sweeps in place
    "3d-bc-nosplit-levels": ("3d", "hgs", _env(BC, NO_SPLIT, NO_DENSE)),
    "3d-hgs-compact": ("3d", "hgs", _env({"AMGX_BGSB_COMPACT": "1"}, NO_DENSE)),     # sweep blocks grown over the graph (gs_block_ids)
    "3d-gs-levels": ("3d", "gs", NO_DENSE),                        # multicolour row list
    "3d-gs-bsell": ("3d", "gs", _env(BSELL, NO_DENSE)),            # multicolour BSELL copy, split where the level allows it
    "3d-gs-bsell-nosplit": ("3d", "gs", _env(BSELL, NO_DENSE, {"AMGX_NO_BGS_SPLIT": "1"})),
    "3d-mixed": ("3d", "mixed", NO_DENSE),                         # hgs on level 0, Chebyshev below
    "rot-hgs-levels": ("rot", "hgs", NO_DENSE),                    # 6x6 everywhere
    "rot-bc-levels": ("rot", "hgs", _env(BC, NO_DENSE)),
    "rot-gs-bsell": ("rot", "gs", _env(BSELL, NO_DENSE)),
    "rot-gs-levels": ("rot", "gs", NO_DENSE),
    "2d-hgs-levels": ("2d", "hgs", NO_DENSE),                      # 2x2 fine, 3x3 coarse
    "2d-bc-levels": ("2d", "hgs", _env(BC, NO_DENSE)),
    "2d-gs-bsell": ("2d", "gs", _env(BSELL, NO_DENSE)),
}
ALL = list(SPECS)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, env=None, **kw):
    """DeviceAMGMatrix created with `env` set in os.environ (restored afterwards: the switches are read at create)"""
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


def _problem(name):
    grid, rot = SHAPES[SPECS[name][0]][:2]
    return elasticity_case(grid, rot, 10)


def _handle(name, **more):
    shape, sm, env = SPECS[name]
    H = _problem(name)[1]
    if sm == "mixed":
        sm = ["hgs"] + ["cheby"] * (H.n_levels - 1)
    return _dev(H, env, sm_type=sm, **more)


def _smoothed(dev):
    d = dev.cycle_info()["dense_level"]
    return range(d if d >= 0 else dev.n_levels - 1)


def _check_forms(name, dev):
    """the handle really is the case its name says (a hierarchy that does not produce the form is a wrong case, not a skip)"""
    shape, sm, env = SPECS[name]
    grid, rot, bs0, rows0, bb0 = SHAPES[shape]
    H = _problem(name)[1]
    assert H.levels[0].A.br == bs0 and H.levels[0].A.n_rows == rows0, (name, H.levels[0].A.br, H.levels[0].A.n_rows)
    dense = dev.cycle_info()["dense_level"]
    if env.get("AMGX_NO_DENSE_TAIL"):
        assert dense < 0 and dev.n_levels >= 3, (name, dense, dev.n_levels)
    else:
        assert dense >= 1, (name, dense)
    lp = [dev.level_paths(l) for l in _smoothed(dev)]
    forms = [p["gs_form"] for p in lp]
    if sm in ("hgs", "mixed"):
        first = "block-coloured" if "AMGX_BGSB_BC_MIN_ROWS" in env else "hybrid-block"
        assert forms[0] == first and lp[0]["gs_block"] == bb0, (name, forms, lp[0])
        assert lp[0]["gs_split"] == (0 if "AMGX_BGSB_NO_SPLIT" in env else 1), (name, lp[0])
        if first == "block-coloured":
            assert lp[0]["gs_block_colors"] >= 2, (name, lp[0])
        if "AMGX_BGSB_COMPACT" in env:
            assert dev.hgs[0]["block_of_row"] is not None, name
        if sm == "mixed":
            assert set(forms[1:]) <= {None}, (name, forms)
            assert [dev.smoother_info(l)["sm_type"] for l in _smoothed(dev)] == ["gs"] + ["cheby"] * (len(forms) - 1)
        else:
            assert set(forms) <= BLOCK_FORMS, (name, forms)
            if dense < 0:
                assert set(forms[1:]) & {"mc-block-rowlist", "mc-block-bsell"}, (name, forms)     # the small levels really sweep
            if shape == "3d" and dense < 0 and "AMGX_BGSB_COMPACT" not in env:
                assert forms[1] == first and lp[1]["gs_block"] == 60 and H.levels[1].A.br == 6, (name, forms, lp[1])
    else:
        want = "mc-block-bsell" if "AMGX_BGS_BSELL_MIN" in env else "mc-block-rowlist"
        assert forms[0] == want and set(forms) <= {"mc-block-bsell", "mc-block-rowlist"}, (name, forms)
        if "AMGX_NO_BGS_SPLIT" in env or want == "mc-block-rowlist":
            assert not any(p["gs_split"] for p in lp), (name, lp)
    return lp


@functools.lru_cache(maxsize=None)
def _block(shape, k=8, seed=0):
    p = elasticity_case(SHAPES[shape][0], SHAPES[shape][1], 10)[0]
    B = np.stack([rhs(p, seed + j) for j in range(k)])
    B.setflags(write=False)
    return B


_ORACLE = {}


def _reference(name, dev):
    """the oracle's cycle on the 8 columns of _block(shape), computed once per configuration of the oracle: the hybrid oracle is
    configured with the blocks, colours and diagonals the handle was created with (tests.hgs_oracle); the variants that differ in
    the split images or the dense tail only share it"""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    shape, sm, env = SPECS[name]
    key = (shape, sm, "AMGX_BGSB_BC_MIN_ROWS" in env, "AMGX_BGSB_COMPACT" in env)
    if key not in _ORACLE:
        H = _problem(name)[1]
        if sm == "gs":
            orc = Oracle(H.levels, sm_type="gs_mc")
        else:
            lv, types = hgs_levels(H.levels, dev.hgs)
            orc = Oracle(lv, sm_type=types)
        X = np.stack([orc.apply(np.array(b)) for b in _block(shape)])
        X.setflags(write=False)
        _ORACLE[key] = X
    return _ORACLE[key]


def _mult(dev, B, interleaved=False, device=False, graph=True, fuse=FUSE):
    """X = C B through MultMulti; B and the result are (k, n) whatever the layout handed to the library"""
    Bin = np.array(B.T if interleaved else B, order="C")
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


def _check_plan(k, plan):
    assert plan["fused"] == 1 and plan["note"] == "", (k, plan)
    assert sum(plan["groups"]) == k and set(plan["groups"]) <= {1, 2, 4}, (k, plan)
    if k >= 2:
        assert max(plan["groups"]) >= 2, plan
    assert plan["work_bytes"] > 0 or k == 1, (k, plan)


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_plan(name):
    dev = _handle(name)
    _check_forms(name, dev)
    for k in range(1, 9):
        _check_plan(k, dev.multi_plan(k, fuse=FUSE))
        info = dev.multi_info(k)
        for fuse in ("gs", True, False):               # without the new bit: what the handle answers today
            plan = dev.multi_plan(k, fuse=fuse)
            assert plan["fused"] == 0 and plan["groups"] == [1] * k, (name, k, fuse, plan)
            assert ("block level" in plan["note"] or "smoother" in plan["note"]) and "level 0" in plan["note"], (name, k, fuse, plan)
            if fuse == "gs":
                assert "Gauss-Seidel on a block level (level 0)" in plan["note"], (name, k, plan)
            assert {key: plan[key] for key in info} == info, (name, k, fuse, plan, info)


def test_plan_work_bytes_are_those_of_a_jacobi_level():
    """no vector beyond the four of a level: the work space of the fused Gauss-Seidel handle is that of a block Jacobi handle"""
    H = _problem("3d-hgs-levels")[1]
    gs = _handle("3d-hgs-levels")
    jac = _dev(H, NO_DENSE, sm_type="jacobi")
    for k in (2, 4, 7, 8):
        assert gs.multi_plan(k, fuse=FUSE)["work_bytes"] == jac.multi_plan(k, fuse=True)["work_bytes"] > 0, k


def _keeps_the_column_loop(dev, p, words):
    for k in (1, 3, 4, 8):
        for fuse in (FUSE, "gs"):
            plan = dev.multi_plan(k, fuse=fuse)
            assert plan["fused"] == 0 and plan["groups"] == [1] * k, (k, fuse, plan)
        note = dev.multi_plan(k, fuse=FUSE)["note"]
        assert all(w in note for w in words), (note, words)
    B = np.stack([rhs(p, j) for j in range(3)])
    assert np.array_equal(_mult(dev, B), _single(dev, B))                  # the flag is never an error
    assert np.array_equal(_mult(dev, B, interleaved=True, device=True), _single(dev, B))


def test_a_bgs_handle_keeps_the_column_loop_under_the_new_flag():
    pb, Hb = elasticity_case((9, 8, 7), False, 5, 0.12)        # (the bgs case of tests/test_gpu_parity.py: aggregates as blocks)
    Hb.build_bgs()
    _keeps_the_column_loop(_dev(Hb, sm_type="bgs"), pb, ("block Gauss-Seidel (bgs)", "level 0"))


@pytest.mark.parametrize("kw,words", [(dict(mg_cycle="W"), ("cycle is not V",)), (dict(mg_cycle="BS"), ("cycle is not V",)),
                                      (dict(sm_steps=2), ("sm_steps > 1 or sm_symm", "level 0"))], ids=["W", "BS", "sm_steps"])
def test_other_cycles_and_smoother_steps_keep_the_column_loop_under_the_new_flag(kw, words):
    p, H = _problem("3d-hgs")
    _keeps_the_column_loop(_dev(H, sm_type="hgs", **kw), p, words)


def test_a_sweep_block_beyond_the_lds_limit_keeps_the_column_loop():
    p, H = _problem("3d-hgs")
    # 2 * 420 * 3 * 4 * 8 + 420 * 4 = 82320 bytes of LDS at width 4: beyond the 64 KB of a launch
    big = _dev(H, {"AMGX_BGSB_ROWS": "420"}, sm_type="hgs")
    assert big.level_paths(0)["gs_form"] == "hybrid-block" and big.level_paths(0)["gs_block"] == 420
    _keeps_the_column_loop(big, p, ("sweep block too large for the multi-vector sweep (level 0)",))
    # ... and the level entry takes the single-vector step there
    n = big.sizes[0]
    rng = np.random.default_rng(2)
    free = np.repeat(p.free, p.bs).astype(np.float64)
    B, X0 = rng.standard_normal((4, n)) * free, rng.standard_normal((4, n)) * free
    one = X0.copy()
    for j in range(4):
        big.Smooth(0, one[j], np.ascontiguousarray(B[j]), np.zeros(n))
    X = X0.copy()
    big.SmoothMulti(0, X, B, fuse=FUSE)
    assert np.array_equal(X, one)


# ---- 2. sweep against sweep, bit for bit ------------------------------------------------------------------------------------
def _smooth_multi(dev, level, X0, B, x_zero, back, interleaved, device, fuse=FUSE):
    Xin = np.array(X0.T if interleaved else X0, order="C")
    Bin = np.array(B.T if interleaved else B, order="C")
    if device:
        import torch
        Xd, Bd = torch.from_numpy(Xin).cuda(), torch.from_numpy(Bin).cuda()
        dev.SmoothMulti(level, Xd, Bd, x_zero=x_zero, back=back, interleaved=interleaved, fuse=fuse)
        torch.cuda.synchronize()
        Xin = Xd.cpu().numpy()
    else:
        dev.SmoothMulti(level, Xin, Bin, x_zero=x_zero, back=back, interleaved=interleaved, fuse=fuse)
    return np.ascontiguousarray(Xin.T) if interleaved else Xin


@pytest.mark.parametrize("name", ALL)
def test_sweep_equals_the_single_vector_sweep(name):
    dev = _handle(name)
    lp = _check_forms(name, dev)
    H = _problem(name)[1]
    rng = np.random.default_rng(3)
    seen = set()
    for level in _smoothed(dev):
        if lp[level]["gs_form"] is None:               # (the Chebyshev levels of the mixed handle)
            continue
        n = dev.sizes[level]
        bs = H.levels[level].A.br
        free = np.repeat(H.levels[level].free, bs).astype(np.float64)
        assert free.size == n
        B = rng.standard_normal((7, n)) * free
        Xs = rng.standard_normal((7, n)) * free
        seen.add((lp[level]["gs_form"], bs, lp[level]["gs_split"]))
        for back in (False, True):
            for x_zero in (False, True):
                X0 = np.zeros_like(Xs) if x_zero else Xs
                one = X0.copy()
                for j in range(7):
                    dev.Smooth(level, one[j], np.ascontiguousarray(B[j]), np.zeros(n), x_zero=x_zero, back=back)
                assert not np.array_equal(one, X0)
                for k in (2, 4, 7):
                    for interleaved in (False, True):
                        for device in (False, True):
                            X = _smooth_multi(dev, level, X0[:k], B[:k], x_zero, back, interleaved, device)
                            assert np.array_equal(X, one[:k]), (name, level, lp[level]["gs_form"], bs, back, x_zero, k, interleaved, device,
                                                                float(np.abs(X - one[:k]).max()))
    print(name, sorted(seen, key=str))


def test_sweep_without_the_new_bit_is_the_column_loop():
    """fuse="gs" on a block level: the level entry answers through the single-vector step, as before"""
    dev = _handle("3d-hgs-levels")
    H = _problem("3d-hgs-levels")[1]
    rng = np.random.default_rng(4)
    n = dev.sizes[0]
    free = np.repeat(H.levels[0].free, 3).astype(np.float64)
    B, X0 = rng.standard_normal((4, n)) * free, rng.standard_normal((4, n)) * free
    one = X0.copy()
    for j in range(4):
        dev.Smooth(0, one[j], np.ascontiguousarray(B[j]), np.zeros(n))
    for fuse in ("gs", True, False, FUSE):
        assert np.array_equal(_smooth_multi(dev, 0, X0, B, False, False, True, True, fuse=fuse), one), fuse


# ---- 3. the cycle against the oracle and against Mult -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_cycle_matches_oracle_and_mult(name):
    dev = _handle(name)
    _check_forms(name, dev)
    B = _block(SPECS[name][0])
    ref = None if SPECS[name][1] == "mixed" else _reference(name, dev)
    one = _single(dev, np.array(B))
    worst = em = 0.0
    for k, interleaved, device, graph in ((8, False, False, True), (2, True, True, True), (7, False, True, False), (4, True, False, True),
                                          (3, False, False, True), (6, True, True, False)):
        _check_plan(k, dev.multi_plan(k, fuse=FUSE))
        X = _mult(dev, B[:k], interleaved, device, graph)
        for j in range(k):
            m = _rel(X[j], one[j])
            em = max(em, m)
            if ref is not None:
                e = _rel(X[j], ref[j])
                worst = max(worst, e)
                assert e <= 1e-10, (name, k, interleaved, device, graph, j, e)
            assert m <= 1e-12, (name, k, interleaved, device, graph, j, m)
        if k in (7, 3):
            assert np.array_equal(X[k - 1], one[k - 1]), (name, k)      # the single column IS the single-vector path
    print(f"{name}: vs oracle {worst:.2e} (1e-10), vs Mult {em:.2e} (1e-12)")


# ---- 4. no cross-talk between the columns -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3d-hgs-levels", "3d-bc-levels", "rot-gs-bsell", "3d-gs-levels", "3d-mixed"])
def test_columns_do_not_talk_to_each_other(name):
    p = _problem(name)[0]
    dev = _handle(name)
    free = np.repeat(p.free, p.bs).astype(bool)
    rng = np.random.default_rng(5)
    B8 = np.array(_block(SPECS[name][0], seed=20))
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
        Bn[k // 2] = np.nan                                     # changing one column of B changes only that column of the result
        Xn = _mult(dev, Bn)
        keep = [j for j in range(k) if j != k // 2]
        assert np.array_equal(Xn[keep], X[keep]), k
        assert np.all(np.isnan(Xn[k // 2][free])), k
        assert np.array_equal(X, X8[:k]), k                     # a column's bits are the same at k = 2, 4 and 8
    assert np.array_equal(_mult(dev, B8[:1]), _single(dev, B8[:1]))
    X7 = _mult(dev, B8[:7])
    assert np.array_equal(X7[6], _single(dev, B8[6:7])[0])
    assert np.array_equal(X7[:4], _mult(dev, B8[:4]))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["3d-hgs-levels", "3d-bc-levels"])
def test_graph_replay_with_changing_k_and_flag_on_the_same_buffers(name, device):
    import torch
    dev = _handle(name)
    n = dev.sizes[0]
    B = np.array(_block(SPECS[name][0])[:4])
    fresh = {fuse: _mult(_handle(name), B, fuse=fuse) for fuse in (FUSE, "gs", True, False)}
    loop = _single(_handle(name), B)
    for fuse in ("gs", True, False):
        assert np.array_equal(fresh[fuse], loop), fuse
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
    steps = [(4, False, FUSE), (2, False, FUSE), (4, False, False), (4, False, FUSE), (4, True, FUSE), (2, True, "gs"), (2, True, FUSE),
             (4, False, True), (3, False, FUSE), (4, True, FUSE), (3, False, "gs"), (4, False, FUSE)]
    for step, (k, il, fuse) in enumerate(steps):
        X = run(k, il, fuse)
        want = fresh[fuse][:k].copy()
        if fuse == FUSE and k == 3:
            want[2] = loop[2]
        assert np.array_equal(X, want), (step, k, il, fuse)
        got[(k, il, fuse)] = X
    for (k, il, fuse), X in got.items():
        assert np.array_equal(run(k, il, fuse, graph=False), X), (k, il, fuse)   # direct launches


# ---- 5. k independent CG recurrences, symmetry --------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["3d-hgs", "3d-bc-levels"])
def test_solve_multi(name, device):
    import torch
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = _problem(name)
    dev = _handle(name)
    assert dev.multi_plan(4, fuse=FUSE)["fused"] == 1 and dev.multi_plan(4, fuse=FUSE)["groups"] == [4]
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
        cg.SolveMulti(torch.from_numpy(lay(B)).cuda(), sol, interleaved=interleaved, fuse=FUSE)
        torch.cuda.synchronize()
        X = sol.cpu().numpy()
    else:
        X = lay(np.zeros_like(B))
        cg.SolveMulti(lay(B), X, interleaved=interleaved, fuse=FUSE)
    X = X.T if interleaved else X
    its, errs = cg.iterations, cg.errors
    assert its[3] == 0 and errs[3] == [0.0] and not X[3].any() and not np.signbit(X[3]).any()
    A = H.levels[0].A.to_scipy()
    f = free.astype(bool)
    for j in range(3):
        one = NativeCGSolver(dev, dev, tol=tol, maxsteps=100)
        one.Solve(np.ascontiguousarray(B[j]))
        print(f"column {j}: iterations multi {its[j]} single {one.iterations}")
        assert abs(its[j] - one.iterations) <= 1, (j, its[j], one.iterations)
        assert len(errs[j]) == its[j] + 1
        m = min(its[j], one.iterations)
        assert np.allclose(errs[j][:m], one.errors[:m], rtol=1e-6, atol=0), j
        assert np.linalg.norm((A @ X[j] - B[j])[f]) <= 1e-8 * np.linalg.norm(B[j]), j


@pytest.mark.parametrize("name", ["3d-hgs-levels", "3d-bc-levels", "rot-gs-bsell", "2d-hgs-levels", "3d-mixed"])
def test_fused_cycle_is_symmetric(name):
    dev = _handle(name)
    B = np.array(_block(SPECS[name][0], seed=40)[:4])
    X = _mult(dev, B, interleaved=True, device=True)
    for u, v in ((0, 1), (2, 3)):
        a, b = float(B[v] @ X[u]), float(B[u] @ X[v])           # v^T C u and u^T C v from one fused call
        assert abs(a - b) <= 1e-10 * abs(a), (name, u, v, a, b)
