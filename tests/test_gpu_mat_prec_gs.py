"""Single-precision images for Gauss-Seidel on block levels (mat_prec = "single_gs", AMGX_PREC_F32 on AMGX_SM_GS levels).

Definition under test: on a Gauss-Seidel level that has the images (level_extra(level)["gs_f32"]), every value of every BSELL image
the sweeps and the residual after the sweep from zero read is that image's fp64 value rounded to float (update_res, the residual of
an iterate that a further correction uses, reads the fp64 A); layout, index arrays, dinv (that of the TRUE A), the
vectors, the LDS contents and the order of additions are those of the fp64 kernels.  Hence
  * the handle equals, BIT FOR BIT, the handle created under AMGX_GS_F32_WIDE=1 (the fp64 kernels on fp64 images that hold the
    rounded values) -- every form, split or not;
  * without the split images (where no image holds anything but entries of A) it equals, bit for bit, a double handle on
    tests/mat_prec_ref.RoundedHierarchy(H, image levels) that is given the smoother data of the true A (hgs_pre), and the oracle in
    the device's sweep order on those levels to 1e-10, the project's bound for Gauss-Seidel in the GPU's order.  (With the split the
    diagonal blocks enter through dinv, i.e. with their TRUE values, and `rest` of the hybrid form stores them scaled: an oracle on
    rounded levels is then another operator, 6e-8 away.)
Every case first asserts, through level_paths / level_extra, that level 0 has the form it names and reads float images.

Measured maxima on an MI355X: see the docstrings of the tests that print them and DESIGN.md 5.17."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.mat_prec_ref import RoundedHierarchy
from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
BC = {"AMGX_BGSB_BC_MIN_ROWS": "0"}
BSELL = {"AMGX_BGS_BSELL_MIN": "1"}
WIDE = {"AMGX_GS_F32_WIDE": "1"}
NO_F32 = {"AMGX_NO_MAT_F32": "1"}

# shape -> (grid, rotations, block size of level 0, block rows of level 0)
SHAPES = {"3d": ((14, 13, 12), False, 3, 2184), "rot": ((12, 11, 10), True, 6, 1320), "2d": ((40, 36), False, 2, 1440)}


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


# form -> (smoother, environment, gs_form of level 0, gs_split of level 0)
FORMS = {
    "hybrid": ("hgs", NO_DENSE, "hybrid-block", 1),
    "hybrid-nosplit": ("hgs", _env(NO_DENSE, {"AMGX_BGSB_NO_SPLIT": "1"}), "hybrid-block", 0),
    "hybrid-compact": ("hgs", _env(NO_DENSE, {"AMGX_BGSB_COMPACT": "1"}), "hybrid-block", 1),
    "bc": ("hgs", _env(NO_DENSE, BC), "block-coloured", 1),
    "bc-nosplit": ("hgs", _env(NO_DENSE, BC, {"AMGX_BGSB_NO_SPLIT": "1"}), "block-coloured", 0),
    "mc": ("gs", _env(NO_DENSE, BSELL), "mc-block-bsell", 1),
    "mc-nosplit": ("gs", _env(NO_DENSE, BSELL, {"AMGX_NO_BGS_SPLIT": "1"}), "mc-block-bsell", 0),
}
NOSPLIT = ["hybrid-nosplit", "bc-nosplit", "mc-nosplit"]
RUNS = ((False, True), (True, True), (True, False), (False, False))      # (device pointers, graph)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(shape):
    grid, rot, bs0, rows0 = SHAPES[shape]
    p, H = elasticity_case(grid, rot, 10)
    assert H.levels[0].A.br == bs0 and H.levels[0].A.n_rows == rows0
    return p, H


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


@functools.lru_cache(maxsize=None)
def _handle(shape, form, prec, extra=(), kw=()):
    """one handle per (shape, form, "single_gs" | "wide" | "double", further environment, further arguments), shared by the tests"""
    sm, env = FORMS[form][:2]
    env = _env(env, dict(extra), WIDE if prec == "wide" else {})
    return _dev(_case(shape)[1], env, sm_type=sm, mat_prec="double" if prec == "double" else "single_gs", **dict(kw))


def _image_levels(dev, form=None):
    """the levels whose sweeps read float images; with `form`: level 0 has that form and is one of them"""
    lv = [l for l in range(dev.n_levels) if dev.level_extra(l)["gs_f32"]]
    for l in lv:
        e = dev.level_extra(l)
        values = dev.matrix_info(l, "A32")
        # (A has the float image where it is BSELL; a small level whose A stayed in block CSR keeps rounded values at fp64 width)
        assert e["gs_f32_images"] >= 2 and e["gs_f32_bytes"] > 0 and values["fmt"] in ("bsell", None), (l, e, values)
    if form is not None:
        lp = dev.level_paths(0)
        assert lp["gs_form"] == FORMS[form][2] and lp["gs_split"] == FORMS[form][3], (form, lp)
        assert lv and lv[0] == 0 and dev.cycle_info()["dense_level"] < 0 and dev.matrix_info(0, "A32")["fmt"] == "bsell", (form, lv)
    return lv


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


def _smooth_inputs(H, dev, level, seed):
    bs = H.levels[level].A.br
    free = np.repeat(H.levels[level].free, bs).astype(np.float64)
    rng = np.random.default_rng(seed)
    n = dev.sizes[level]
    return rng.standard_normal(n) * free, rng.standard_normal(n) * free


def _smooth_all(dev, H, level, x0, b, device=False):
    """x and res of Smooth / SmoothBack under the eight flag combinations"""
    out = []
    r0 = np.zeros_like(b)
    dev.Residual(level, x0, b, r0)
    for back in (False, True):
        for ru in (False, True):
            for ur in (False, True):
                for xz in (False, True):
                    x = np.zeros_like(x0) if xz else x0.copy()
                    r = (b.copy() if xz else r0.copy()) if ru else np.zeros_like(b)
                    if device:
                        import torch
                        xd, bd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(r).cuda()
                        dev.Smooth(level, xd, bd, rd, res_updated=ru, update_res=ur, x_zero=xz, back=back)
                        torch.cuda.synchronize()
                        x, r = xd.cpu().numpy(), rd.cpu().numpy()
                    else:
                        dev.Smooth(level, x, b, r, res_updated=ru, update_res=ur, x_zero=xz, back=back)
                    out.append(x)
                    if ur:
                        out.append(r)
    return out


# ---- 1. bit for bit: the float kernels against the fp64 kernels on images that hold the rounded values ------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_against_the_wide_twin(shape, form):
    p, H = _case(shape)
    single, wide, double = _handle(shape, form, "single_gs"), _handle(shape, form, "wide"), _handle(shape, form, "double")
    lv = _image_levels(single, form)
    for l in range(single.n_levels):
        es, ew, ed = single.level_extra(l), wide.level_extra(l), double.level_extra(l)
        assert ew["gs_f32"] == 0 and ew["gs_f32_images"] == es["gs_f32_images"] and es["gs_f32_bytes"] <= ew["gs_f32_bytes"] <= 2 * es["gs_f32_bytes"], (l, es, ew)
        if l == 0:
            assert ew["gs_f32_bytes"] == 2 * es["gs_f32_bytes"], (es, ew)           # 8 instead of 4 bytes per value
        assert (ed["gs_f32"], ed["gs_f32_images"], ed["gs_f32_bytes"]) == (0, 0, 0) and double.matrix_info(l, "A32")["fmt"] is None
        assert single.level_paths(l) == wide.level_paths(l) == double.level_paths(l), l
    b = rhs(p, 3)
    want = _mult(wide, b)
    assert np.isfinite(want).all() and np.linalg.norm(want) > 0 and not np.array_equal(want, _mult(double, b))
    for device, graph in RUNS:
        got = _mult(single, b, device, graph)
        assert np.array_equal(got, want), (shape, form, device, graph, _rel(got, want))
    seen = set()
    for level in (0, 1):
        if level not in lv:
            continue
        seen.add((single.level_paths(level)["gs_form"], H.levels[level].A.br))
        x0, bb = _smooth_inputs(H, single, level, 7 + level)
        a, w = _smooth_all(single, H, level, x0, bb), _smooth_all(wide, H, level, x0, bb)
        for i, (u, v) in enumerate(zip(a, w)):
            assert np.array_equal(u, v), (shape, form, level, i, _rel(u, v))
        for i, (u, v) in enumerate(zip(_smooth_all(single, H, level, x0, bb, device=True), w)):
            assert np.array_equal(u, v), (shape, form, level, i, "device pointers")
        assert any(not np.array_equal(u, v) for u, v in zip(a, _smooth_all(double, H, level, x0, bb)))
    print(shape, form, "image levels", lv, sorted(seen, key=str))
    assert (FORMS[form][2], SHAPES[shape][2]) in seen


@pytest.mark.parametrize("kw", [dict(mg_cycle="W"), dict(mg_cycle="BS"), dict(sm_steps=2), dict(sm_symm=True), dict(sm_steps=2, sm_symm=True)],
                         ids=["W", "BS", "steps2", "symm", "steps2-symm"])
@pytest.mark.parametrize("form", ["hybrid", "bc", "mc", "hybrid-nosplit"])
def test_bitwise_other_cycles_and_the_proxy_smoother(form, kw):
    p, H = _case("3d")
    key = tuple(sorted(kw.items()))
    single, wide = _handle("3d", form, "single_gs", (), key), _handle("3d", form, "wide", (), key)
    _image_levels(single, form)
    b = rhs(p, 4)
    want = _mult(wide, b)
    for device, graph in RUNS:
        assert np.array_equal(_mult(single, b, device, graph), want), (form, kw, device, graph)
    x0, bb = _smooth_inputs(H, single, 0, 11)
    for u, v in zip(_smooth_all(single, H, 0, x0, bb), _smooth_all(wide, H, 0, x0, bb)):
        assert np.array_equal(u, v), (form, kw)
    # SmoothVFromLevel: the sub-cycle from level 1 as a smoother
    n1 = single.sizes[1]
    x1, b1 = _smooth_inputs(H, single, 1, 12)
    res = []
    for dev in (single, wide):
        x, r = x1.copy(), np.zeros(n1)
        dev.SmoothVFromLevel(1, x, b1, r, False, True, False)
        res.append((x, r))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (form, kw)


@pytest.mark.parametrize("xmode", range(6))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_in_every_gather_mode_of_the_off_image(shape, xmode):
    """AMGX_BSELL_XMODE 0 .. 5 rearrange the gathers of the OFF stream (and of the BSELL products): same arithmetic in every mode"""
    p, H = _case(shape)
    extra = (("AMGX_BSELL_XMODE", str(xmode)),)
    b = rhs(p, 5)
    for form in ("hybrid", "bc"):
        single, wide = _handle(shape, form, "single_gs", extra), _handle(shape, form, "wide", extra)
        _image_levels(single, form)
        want = _mult(wide, b)
        assert np.array_equal(_mult(single, b), want), (shape, form, xmode)
        assert np.array_equal(_mult(single, b, True, False), want), (shape, form, xmode)
        assert np.array_equal(want, _mult(_handle(shape, form, "single_gs"), b)), (shape, form, xmode)      # ... and that of mode 0
        x0, bb = _smooth_inputs(H, single, 0, 13)
        for u, v in zip(_smooth_all(single, H, 0, x0, bb), _smooth_all(wide, H, 0, x0, bb)):
            assert np.array_equal(u, v), (shape, form, xmode)


# ---- 2. / 3. the definition: an independent rounding, and the oracle -------------------------------------------------------------
def _rounded(H, single, lv):
    """RoundedHierarchy(H, lv) whose hybrid levels carry the smoother data the single handle was created with (from the TRUE A)"""
    import copy
    RH = RoundedHierarchy(H, lv)
    for i, info in enumerate(single.hgs):
        if info is not None and info.get("block_color") is None and info.get("block_of_row") is None:
            L = copy.copy(RH.levels[i])
            L.hgs_pre = dict(B=info["B"], color=info["color"], n_colors=info["n_colors"], dinv=info["dinv"])
            RH.levels[i] = L
    return RH


@pytest.mark.parametrize("form", NOSPLIT)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_against_a_double_handle_on_rounded_levels_and_the_oracle(shape, form):
    """Oracle maxima measured on an MI355X (the print of every case): 1.7e-16 ... 2.3e-15 over the nine shape / form pairs (bound 1e-10)."""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    p, H = _case(shape)
    sm, env = FORMS[form][:2]
    single = _handle(shape, form, "single_gs")
    lv = _image_levels(single, form)
    RH = _rounded(H, single, lv)
    assert not np.array_equal(np.asarray(RH.levels[0].A.val), np.asarray(H.levels[0].A.val)) and RH.levels[0].dinv is H.levels[0].dinv
    double = _dev(RH, env, sm_type=sm)
    assert _image_levels(double) == [] and [double.level_paths(l) for l in range(H.n_levels)] == [single.level_paths(l) for l in range(H.n_levels)]
    for i, (a, c) in enumerate(zip(single.hgs, double.hgs)):
        assert (a is None) == (c is None), i
        if a is not None:
            assert np.array_equal(a["dinv"], c["dinv"]) and np.array_equal(a["color"], c["color"]) and a["B"] == c["B"], i
    B = [rhs(p, s) for s in (3, 8)]
    for b in B:
        want = _mult(double, b)
        for device, graph in RUNS:
            got = _mult(single, b, device, graph)
            assert np.array_equal(got, want), (shape, form, device, graph, _rel(got, want))
    for level in [l for l in (0, 1) if l in lv]:
        x0, bb = _smooth_inputs(H, single, level, 17 + level)
        # (the sweep reads the float images; update_res is the residual of an iterate that a further correction uses and reads the TRUE
        # A, as amgx_residual does -- the rounded double handle reads its rounded A there)
        for back in (False, True):
            for xz in (False, True):
                xs, xd = (np.zeros_like(x0) if xz else x0.copy()), (np.zeros_like(x0) if xz else x0.copy())
                rs, rd, rt = np.zeros_like(bb), np.zeros_like(bb), np.zeros_like(bb)
                single.Smooth(level, xs, bb, rs, update_res=True, x_zero=xz, back=back)
                double.Smooth(level, xd, bb, rd, update_res=True, x_zero=xz, back=back)
                single.Residual(level, xs, bb, rt)
                assert np.array_equal(xs, xd) and np.array_equal(rs, rt), (shape, form, level, back, xz)
                assert not np.array_equal(rs, rd) and _rel(rs, rd) <= 1e-5, (shape, form, level, back, xz)
    # the oracle in the device's order on the rounded levels, dinv of the true A
    if sm == "gs":
        orc = Oracle(RH.levels, sm_type="gs_mc")
    else:
        olv, types = hgs_levels(RH.levels, single.hgs)
        orc = Oracle(olv, sm_type=types)
    worst = 0.0
    for b in B:
        e = _rel(_mult(single, b), orc.apply(np.array(b)))
        worst = max(worst, e)
    print(f"{shape} {form}: vs oracle on rounded levels {worst:.2e} (1e-10)")
    assert worst <= 1e-10, (shape, form, worst)


# ---- 4. the rounding is there ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_rounding_is_there_and_small(shape, cycle):
    """|Mult single - Mult double| / |Mult double| in [1e-10, 1e-6] in every form and cycle.

    Measured on an MI355X (the prints below; smallest ... largest over the forms):
                V                      W                      BS
        3d      2.7e-8 ... 4.5e-8      2.9e-8 ... 3.6e-8      2.9e-8 ... 3.5e-8
        rot     3.3e-8 ... 3.7e-8      4.1e-8 ... 4.4e-8      4.1e-8 ... 4.4e-8
        2d      3.7e-8 ... 5.1e-8      4.6e-8 ... 4.9e-8      4.6e-8 ... 4.9e-8
    The W / BS figures rest on update_res reading the fp64 A (Handle::base_smooth): those cycles form the residual of an iterate
    that is close to the solution and correct it again, so a residual from the rounded A would pull the result towards the
    solution of the rounded system -- cond(A) * 6e-8.  With the float image of A in update_res the 2-D shape moved 3.4e-6 (W) and
    3.8e-6 (BS), and the CPU oracle on tests/mat_prec_ref.rounded_levels gives 3.3e-6 / 3.7e-6 for the same right-hand sides."""
    p, H = _case(shape)
    b = rhs(p, 3)
    kw = () if cycle == "V" else (("mg_cycle", cycle),)
    lo, hi = np.inf, 0.0
    for form in (FORMS if cycle == "V" else ("hybrid", "bc", "mc")):
        single, double = _handle(shape, form, "single_gs", (), kw), _handle(shape, form, "double", (), kw)
        _image_levels(single, form)
        e = _rel(_mult(single, b), _mult(double, b))
        print(f"{shape} {form} {cycle}: change {e:.2e}")
        lo, hi = min(lo, e), max(hi, e)
    print(f"{shape} {cycle}: change of one application {lo:.2e} ... {hi:.2e}")
    assert 1e-10 <= lo and hi <= 1e-6, (shape, cycle, lo, hi)


# ---- 5. PCG -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["hybrid", "bc", "mc"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pcg(shape, form):
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = _case(shape)
    single, double = _handle(shape, form, "single_gs"), _handle(shape, form, "double")
    _image_levels(single, form)
    A = H.levels[0].A.to_scipy()
    free = np.repeat(np.asarray(p.free), p.bs).astype(bool)
    b = rhs(p, 3)
    its, res = {}, {}
    for key, dev in (("single", single), ("double", double)):
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
        cg.Solve(b)
        its[key] = cg.iterations
        assert cg.errors[-1] <= 1e-8 * cg.errors[0], (shape, form, key)
        cg = NativeCGSolver(dev, dev, tol=1e-12, maxsteps=100)
        x = np.asarray(cg.Solve(b))
        assert cg.errors[-1] <= 1e-12 * cg.errors[0], (shape, form, key)
        res[key] = np.linalg.norm((b - A @ x)[free]) / np.linalg.norm(b)
    print(f"{shape} {form}: iterations to 1e-8 single {its['single']} double {its['double']} | true residual at 1e-12 "
          f"single {res['single']:.2e} double {res['double']:.2e}")
    assert abs(its["single"] - its["double"]) <= 1, (shape, form, its)
    assert res["single"] <= 10.0 * res["double"], (shape, form, res)


# ---- 6. what stays fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["hybrid", "bc", "mc"])
def test_operator_products_read_the_fp64_image(form):
    p, H = _case("3d")
    single, double = _handle("3d", form, "single_gs"), _handle("3d", form, "double")
    lv = _image_levels(single, form)
    for level in lv[:2]:
        x, b = _smooth_inputs(H, single, level, 21 + level)
        out = []
        for dev in (single, double):
            y, r = np.zeros_like(x), np.zeros_like(x)
            dev.MatVec(level, x, y)
            dev.Residual(level, x, b, r)
            X = np.ascontiguousarray(np.stack([x, b, x + b]))
            Y = np.full_like(X, np.nan)
            dev.MatVecMulti(level, X, Y)
            out.append((y, r, Y))
        for u, v in zip(*out):
            assert np.array_equal(u, v), (form, level)
        A = H.levels[level].A.to_scipy()
        assert _rel(out[0][0], A @ x) <= 1e-13, (form, level)                 # the TRUE A, not the rounded one (6e-8)


@pytest.mark.parametrize("form", ["hybrid", "bc", "mc", "hybrid-nosplit"])
def test_kill_switch_gives_the_double_handle(form):
    p, H = _case("3d")
    sm, env = FORMS[form][:2]
    on, double = _handle("3d", form, "single_gs"), _handle("3d", form, "double")
    _image_levels(on, form)
    for more in (NO_F32, _env(NO_F32, WIDE)):
        off = _dev(H, _env(env, more), sm_type=sm, mat_prec="single_gs")
        assert _image_levels(off) == [] and all(off.level_extra(l)["gs_f32_images"] == 0 for l in range(H.n_levels))
        b = rhs(p, 3)
        want = _mult(double, b)
        for device, graph in RUNS:
            assert np.array_equal(_mult(off, b, device, graph), want), (form, device, graph)
        x0, bb = _smooth_inputs(H, off, 0, 23)
        for u, v in zip(_smooth_all(off, H, 0, x0, bb), _smooth_all(double, H, 0, x0, bb)):
            assert np.array_equal(u, v), form
        assert not np.array_equal(_mult(on, b), want)


# ---- 7. the fused multi-vector sweeps read fp64 images --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["hybrid", "bc", "mc"])
def test_a_single_precision_handle_is_not_fused(form):
    p, H = _case("3d")
    single, wide, double = _handle("3d", form, "single_gs"), _handle("3d", form, "wide"), _handle("3d", form, "double")
    _image_levels(single, form)
    B = np.ascontiguousarray(np.stack([rhs(p, j) for j in range(5)]))
    for dev in (single, wide):
        for k in (1, 2, 4, 5):
            plan = dev.multi_plan(k, fuse="gs_block")
            assert plan["fused"] == 0 and plan["groups"] == [1] * k, (form, k, plan)
            assert "single-precision Gauss-Seidel images (level 0)" in plan["note"], plan
        for k, interleaved in ((2, False), (5, True), (4, False)):
            Bin = np.array(B[:k].T if interleaved else B[:k], order="C")
            X = np.full_like(Bin, np.nan)
            dev.MultMulti(Bin, X, interleaved=interleaved, fuse="gs_block")
            X = X.T if interleaved else X
            for j in range(k):
                assert np.array_equal(X[j], _mult(dev, np.ascontiguousarray(B[j]))), (form, k, j)
    # a column of SmoothMulti is Smooth, bit for bit
    x0, bb = _smooth_inputs(H, single, 0, 25)
    X, Bm = np.ascontiguousarray(np.stack([x0, 2 * x0, bb])), np.ascontiguousarray(np.stack([bb, bb, x0]))
    one = X.copy()
    for j in range(3):
        single.Smooth(0, one[j], np.ascontiguousarray(Bm[j]), np.zeros_like(bb))
    single.SmoothMulti(0, X, Bm, fuse="gs_block")
    assert np.array_equal(X, one), form
    # the double handle stays fused
    plan = double.multi_plan(4, fuse="gs_block")
    assert plan["fused"] == 1 and plan["note"] == "" and plan["groups"] == [4], plan


# ---- 8. mixed hierarchy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,first", [("3d", "hgs"), ("rot", "hgs"), ("3d", "cheby")])      # (level 1 of "rot" is too small for sweep blocks)
def test_mixed_hierarchy_has_images_on_both_kinds_of_level(shape, first):
    """hgs on level 0 and Chebyshev below; and the other way round, because level 1 of these shapes keeps A in block CSR -- a
    Chebyshev level there stays fp64 silently while a hybrid-block level still has its BSELL sweep images"""
    p, H = _case(shape)
    n = H.n_levels
    types = ["hgs"] + ["cheby"] * (n - 1) if first == "hgs" else ["cheby", "hgs"] + ["cheby"] * (n - 2)
    gs_level = 0 if first == "hgs" else 1
    lm = [2.5] * n
    single = _dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm, mat_prec="single_gs")
    wide = _dev(H, _env(NO_DENSE, WIDE), sm_type=types, cheb_lambda_max=lm, mat_prec="single_gs")
    cheb_only = _dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm, mat_prec="single")
    double = _dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm)
    assert _image_levels(single) == [gs_level] and single.level_paths(gs_level)["gs_form"] == "hybrid-block"
    a32 = [single.matrix_info(l, "A32")["fmt"] for l in range(n)]
    c32 = [cheb_only.matrix_info(l, "A32")["fmt"] for l in range(n)]
    assert a32[0] == "bsell" and a32[-1] is None, a32
    assert _image_levels(cheb_only) == [] and c32[gs_level] is None, c32
    assert [f for l, f in enumerate(a32) if l != gs_level] == [f for l, f in enumerate(c32) if l != gs_level], (a32, c32)
    if first == "cheby":
        assert c32[0] == "bsell"                                   # images on both kinds of level: Chebyshev on 0, Gauss-Seidel on 1
    b = rhs(p, 3)
    xs, xw, xc, xd = _mult(single, b), _mult(wide, b), _mult(cheb_only, b), _mult(double, b)
    assert np.array_equal(xs, xw)
    assert not np.array_equal(xs, xc) and np.array_equal(xc, xd) == (not any(c32))
    assert 1e-10 <= _rel(xs, xd) <= 1e-6 and _rel(xs, xc) <= 1e-6
    per_level = ["single"] * n
    per_level[gs_level] = "single_gs"
    assert np.array_equal(_mult(_dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm, mat_prec=per_level), b), xs)


# ---- 9. levels without images, errors, the timing hook -------------------------------------------------------------------------
def test_scalar_and_row_list_levels_stay_fp64():
    ps, Hs = poisson_case((17, 17, 17), "right|top", 20)
    b = rhs(ps, 3)
    for sm in ("hgs", "gs"):
        single, double = _dev(Hs, NO_DENSE, sm_type=sm, mat_prec="single_gs"), _dev(Hs, NO_DENSE, sm_type=sm)
        assert _image_levels(single) == [] and all(single.matrix_info(l, "A32")["fmt"] is None for l in range(Hs.n_levels))
        for device, graph in RUNS:
            assert np.array_equal(_mult(single, b, device, graph), _mult(double, b)), (sm, device, graph)
    # block levels whose multicolour sweep walks the row list over block CSR: no image, silently
    p, H = _case("3d")
    single, double = _dev(H, NO_DENSE, sm_type="gs", mat_prec="single_gs"), _dev(H, NO_DENSE, sm_type="gs")
    assert single.level_paths(0)["gs_form"] == "mc-block-rowlist" and _image_levels(single) == []
    assert np.array_equal(_mult(single, rhs(p, 3)), _mult(double, rhs(p, 3)))
    # the stand-alone smoother passes the argument through (a scalar matrix: no image)
    from ngsamg_amd import NgsAMG
    from tests.problems import to_matrix
    rng = np.random.default_rng(1)
    x0, bb = rng.standard_normal(ps.n) * ps.free, rng.standard_normal(ps.n) * ps.free
    out = []
    for prec in ("double", "single_gs"):
        sm = NgsAMG.CreateHybridGSS(to_matrix(ps), ps.free, mat_prec=prec)
        x, r = x0.copy(), np.zeros(ps.n)
        sm.Smooth(x, bb, r, False, True, False)
        out.append((x, r))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_c_abi_errors():
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.device import hierarchy_desc
    lib = _lib.hip()
    p, H = _case("3d")
    pb, Hb = elasticity_case((9, 8, 7), False, 5, 0.12)
    Hb.build_bgs()
    for hier, sm in ((H, "jacobi"), (Hb, "bgs")):
        desc, keep, _ = hierarchy_desc(hier, sm_type=sm)
        desc.levels[0].mat_prec = _lib.AMGX_PREC_F32
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, sm
        msg = lib.amgx_last_error(None).decode()
        assert "level 0" in msg and "mat_prec = AMGX_PREC_F32" in msg and "Gauss-Seidel" in msg, msg
    # a Gauss-Seidel block level takes the value, and the coarsest level ignores it
    desc, keep, _ = hierarchy_desc(H, sm_type="hgs")
    for l in range(H.n_levels):
        desc.levels[l].mat_prec = _lib.AMGX_PREC_F32
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) == 0, lib.amgx_last_error(None).decode()
    out = np.zeros(12, dtype=np.int64)
    assert lib.amgx_level_extra(h, 0, out.ctypes.data_as(_lib.c_i64p), 12) == 0 and out[9] == 1 and out[10] >= 3 and out[11] > 0, out
    fmt, stored, lanes = C.c_int32(), C.c_int64(), C.c_int32()
    assert lib.amgx_matrix_info(h, 0, 7, C.byref(fmt), C.byref(stored), C.byref(lanes)) == 0 and fmt.value == 2
    assert lib.amgx_matrix_info(h, 0, 8, C.byref(fmt), C.byref(stored), C.byref(lanes)) != 0
    lib.amgx_destroy(h)
    # a value beyond the range of float: the error names the level, for the float images and for the wide twin
    A = H.levels[0].A
    val = np.array(A.val, dtype=np.float64)
    val[7 * A.br * A.br + 1] = 1e39
    import dataclasses
    bad = RoundedHierarchy(H, [])
    bad.levels[0] = dataclasses.replace(H.levels[0], A=Matrix(A.n_rows, A.n_cols, A.br, A.bc, A.rowptr, A.col, val))
    for form in ("hybrid", "bc", "mc"):
        sm, env = FORMS[form][:2]
        for more in ({}, WIDE):
            with pytest.raises(_lib.NgsAMGError, match="single precision") as ei:
                _dev(bad, _env(env, more), sm_type=sm, mat_prec="single_gs")
            assert "level 0" in str(ei.value), str(ei.value)
        _dev(bad, _env(env, NO_F32), sm_type=sm, mat_prec="single_gs")           # ignored request: the double handle takes the matrix


@pytest.mark.parametrize("form", ["hybrid", "bc", "mc"])
def test_time_op_of_the_block_sweep(form):
    """amgx_time_op op 11: HIP events around the backward block sweep of a level while whole cycles run (op 9 of the scalar levels)"""
    import torch
    from ngsamg_amd import _lib
    p, H = _case("3d")
    sm, env = FORMS[form][:2]
    b = torch.from_numpy(rhs(p, 6)).cuda()
    s = torch.cuda.Stream()                                                # (the probe needs a stream that is not the default one)
    with torch.cuda.stream(s):
        for prec in ("single_gs", "double"):
            dev = _dev(H, env, sm_type=sm, mat_prec=prec)
            assert _image_levels(dev, form if prec == "single_gs" else None) == ([] if prec == "double" else _image_levels(dev))
            x0 = torch.empty_like(b); dev.Mult(b, x0)
            s.synchronize()
            for level in (0, 1):
                assert 0.0 < dev.time_op(level, 11, reps=2) < 50.0, (form, prec, level)
            assert dev.time_op(0, 0, reps=2) > 0.0
            with pytest.raises(_lib.NgsAMGError, match="no block Gauss-Seidel sweep"):
                dev.time_op(H.n_levels - 1, 11, reps=2)
            with pytest.raises(_lib.NgsAMGError, match="unknown op"):
                dev.time_op(0, 12, reps=2)
            x1 = torch.empty_like(b); dev.Mult(b, x1)
            s.synchronize()
            assert torch.equal(x0, x1)                                     # the hook leaves a working handle behind
        ps, Hs = poisson_case((17, 17, 17), "right|top", 20)
        with pytest.raises(_lib.NgsAMGError, match="no block Gauss-Seidel sweep"):
            _dev(Hs, NO_DENSE, sm_type="hgs").time_op(0, 11, reps=2)
