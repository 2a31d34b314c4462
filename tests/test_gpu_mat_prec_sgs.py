"""Single-precision images for Gauss-Seidel on SCALAR levels (mat_prec = "single_gs_all", AMGX_PREC_F32_SCALAR_GS).

Definition under test: on a scalar Gauss-Seidel level that has the images (gs_prec_info(level)["f32"]) every value of every image the
sweeps and the residual after the sweep from zero read -- block-hybrid: full, fullLW, lowin, rest, restLW; multicolour: sell, lower,
upper; A itself on a level without split images -- is that image's fp64 value rounded to float; index arrays, dinv and cvec (those of
the TRUE A), the vectors, the LDS contents and the order of additions are those of the fp64 kernels.  Hence
  * the handle equals, BIT FOR BIT, the handle created under AMGX_GS_F32_WIDE=1 (the fp64 kernels on fp64 images that hold the
    rounded values) -- every kernel instantiation, split or not;
  * without the split images it equals, bit for bit, a double handle on tests/mat_prec_ref.RoundedHierarchy(H, image levels) that
    carries the smoother data of the true A (hgs_pre), and the oracle in the device's sweep order on those levels to 1e-10, the
    project's bound for Gauss-Seidel in the GPU's order.  (With the split the diagonal acts through dinv / cvec with its TRUE value.)
Every case first asserts, through gs_prec_info and level_paths, that level 0 has the form it names and reads float images.

Change of one application against the double handle: lower bound 1e-10 (the rounding is there), upper bound 1.3e-6 = 10 x the largest
value tests/test_mat_prec_sgs_cpu.py measures on the same grids (1.29e-7 at (33, 33) multicolour; the factor 10 is the allowance of
DESIGN.md 5.20 for the split forms, which keep the true diagonal).  Measured on an MI355X: see test_the_rounding_is_there_and_small."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import reorder as R
from tests.mat_prec_ref import RoundedHierarchy
from tests.problems import poisson_case, rhs

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": "1"}
WIDE = {"AMGX_GS_F32_WIDE": "1"}
NO_F32 = {"AMGX_NO_MAT_F32": "1"}
NO_SPLIT = {"AMGX_GSB_NO_SPLIT": "1"}
RUNS = ((False, True), (True, True), (True, False), (False, False))      # (device pointers, graph)
LANE_LENGTHS = {1: 17, 2: 32, 4: 64, 8: 128, 16: 256}                    # one longest row per G (tests/test_gpu_gs_paths.py)
GRIDS = {"3d": ((17, 17, 17), "right|top", 20), "2d": ((33, 33), "left|top", 5), "3d-odd": ((24, 22, 20), "right|top", 20)}
CHANGE_MAX = 10 * 1.29e-7
SEEN_DOWN = set()                                                        # level_paths entry 33 of the twin cases that ran


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


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


def _pair(H, env, sm, **kw):
    """the handle with float images and its AMGX_GS_F32_WIDE twin"""
    return (_dev(H, env, sm_type=sm, mat_prec="single_gs_all", **kw), _dev(H, _env(env, WIDE), sm_type=sm, mat_prec="single_gs_all", **kw))


@functools.lru_cache(maxsize=None)
def _grid(name):
    return poisson_case(*GRIDS[name])


@functools.lru_cache(maxsize=None)
def _handle(grid, sm, prec, extra=(), kw=()):
    """one handle per (grid, smoother, "single_gs_all" | "wide" | "double", further environment, further arguments)"""
    env = _env(NO_DENSE, dict(extra), WIDE if prec == "wide" else {})
    return _dev(_grid(grid)[1], env, sm_type=sm, mat_prec="double" if prec == "double" else "single_gs_all", **dict(kw))


def _float_level(single, form, level=0, wide=None):
    """`level` has the sweep form `form` and its sweeps read float images: the images the form and its paths imply"""
    lp, info, ex = single.level_paths(level), single.gs_prec_info(level), single.level_extra(level)
    assert lp["gs_form"] == form, (level, lp)
    assert info["f32"] == 1 and info["wide"] == 0 and info["bytes"] > 0, (level, info)
    if form == "hybrid":
        want = {"full"} | ({"lowin", "rest"} if lp["gs_split"] else {"A"}) | ({"fullLW"} if lp["gs_lw"] else set())
        want |= {"restLW"} if lp["gs_down"] == "sell-lw" else set()
        allowed = want | {"restLW"}
    else:
        want = {"sell"} | ({"lower", "upper"} if lp["gs_split"] else {"A"})
        allowed = want
    assert want <= set(info["images"]) <= allowed, (level, lp, info)
    assert ex["gs_f32"] == 1 and ex["gs_f32_images"] == len(info["images"]) and ex["gs_f32_bytes"] == info["bytes"], (level, ex, info)
    if lp["gs_split"]:
        assert info["released"] > info["bytes"], (level, info)                  # more fp64 bytes given back than float bytes added
    assert (single.matrix_info(level, "A32")["fmt"] is not None) == ("A" in info["images"] and single.matrix_info(level, "A")["fmt"] == "sell"
                                                                      and single.matrix_info(level, "A32")["fmt"] == "sell"), (level, info)
    if wide is not None:
        iw, ew = wide.gs_prec_info(level), wide.level_extra(level)
        assert iw["f32"] == 0 and iw["wide"] == 1 and iw["mask"] == info["mask"] and iw["released"] == 0 and iw["bytes"] >= info["bytes"], (iw, info)
        assert ew["gs_f32"] == 0 and ew["gs_f32_images"] == ex["gs_f32_images"], (ew, ex)
        assert wide.level_paths(level) == lp, level
    return lp


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


def _smooth_all(dev, level, x0, b, device=False):
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


def _inputs(free, n, seed):
    fr = np.asarray(free, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * fr, rng.standard_normal(n) * fr


def _twin_operations(single, wide, free, seed, what, device_smooth=False):
    """Mult (capture, replay, direct launches; host and device pointers) and Smooth forward / backward under the eight flag
    combinations: the float handle equals the twin bit for bit"""
    n = single.sizes[0]
    x0, b = _inputs(free, n, seed)
    want = _mult(wide, b)
    assert np.isfinite(want).all() and np.linalg.norm(want) > 0, what
    for device, graph in RUNS:
        got = _mult(single, b, device, graph)
        assert np.array_equal(got, want), (what, device, graph, _rel(got, want))
    assert np.array_equal(_mult(single, b), want), (what, "replay")
    w = _smooth_all(wide, 0, x0, b)
    for i, (u, v) in enumerate(zip(_smooth_all(single, 0, x0, b), w)):
        assert np.array_equal(u, v), (what, i, _rel(u, v))
    if device_smooth:
        for i, (u, v) in enumerate(zip(_smooth_all(single, 0, x0, b, device=True), w)):
            assert np.array_equal(u, v), (what, i, "device pointers")
    SEEN_DOWN.add(single.level_paths(0)["gs_down"])


# ---- 1. bit for bit against the AMGX_GS_F32_WIDE twin: every kernel instantiation (the shapes of tests/test_gpu_gs_paths.py) --------
@pytest.mark.parametrize("kind", R.GS_ORDERS)
@pytest.mark.parametrize("L", R.GS_LENGTHS)
def test_twin_hybrid_lengths_and_orders(L, kind):
    """G = 1 ... 16 from the longest row, the mid-width and the WP 8 general sweep, the narrow and the WP 8 sweep from zero"""
    A, B, free, H = R.gs_scalar_case(L, kind)
    single, wide = _pair(H, {}, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_split"] == 1 and lp["gs_lw"] == 0
    _twin_operations(single, wide, free, L, (L, kind), device_smooth=(kind == "identity"))


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_twin_hybrid_threads(G, threads):
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], "identity")
    single, wide = _pair(H, {"AMGX_GSB_THREADS": str(threads), "AMGX_GSB_THREADS_MULTI": str(threads)}, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_lanes"] == G and lp["gs_threads"] == threads
    _twin_operations(single, wide, free, threads + G, (G, threads))


@pytest.mark.parametrize("kind", ["identity", "random"])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_twin_hybrid_no_split(G, kind):
    """AMGX_GSB_NO_SPLIT: the sweep from zero reads `full`, the residual after it the image of A"""
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], kind)
    single, wide = _pair(H, NO_SPLIT, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_split"] == 0 and "A" in single.gs_prec_info(0)["images"]
    _twin_operations(single, wide, free, 7 * G, (G, kind))


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("L", [32, 33, 64, 65, 128, 129, 256])
def test_twin_hybrid_local_window(L, cap):
    """AMGX_GSB_LW=1: the general sweep reads the float local-window image, with and without blocks that keep 32-bit columns"""
    A, B, free, H = R.gs_scalar_case(L, "identity")
    env = _env({"AMGX_GSB_LW": "1", "AMGX_LW_MIN_ROWS": "0"}, {"AMGX_LW_TEST_CAP": str(3 * L)} if cap else {})
    single, wide = _pair(H, env, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_lw"] == 1 and lp["gs_mid"] == (L in (33, 65, 129)) and "fullLW" in single.gs_prec_info(0)["images"], lp
    assert (lp["gs_lw_no_window"] > 0) == cap, lp
    _twin_operations(single, wide, free, 11 * lp["gs_lanes"] + cap, (L, cap))


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("L", [33, 65, 129, 256])
def test_twin_hybrid_local_window_threads(L, threads):
    """the local-window sweep at 512 and 1024 lanes (the mid-width float form at 1024 lanes has launch bounds of its own)"""
    A, B, free, H = R.gs_scalar_case(L, "identity")
    single, wide = _pair(H, {"AMGX_GSB_LW": "1", "AMGX_LW_MIN_ROWS": "0", "AMGX_GSB_THREADS_MULTI": str(threads)}, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_lw"] == 1 and lp["gs_threads"] == threads, lp
    _twin_operations(single, wide, free, L + threads, (L, threads))


@pytest.mark.parametrize("L", [17, 32, 64, 128, 256])
def test_twin_hybrid_non_free_rows(L):
    """40 scattered non-free rows and one whole non-free block; 6037 rows are no multiple of B"""
    A, B, free, H = R.gs_scalar_case(L, "identity", True)
    assert A.shape[0] % B != 0 and not free[3 * B:4 * B].any()
    single, wide = _pair(H, {}, "hgs")
    _float_level(single, "hybrid", wide=wide)
    _twin_operations(single, wide, free, L, L)


def test_twin_hybrid_single_partial_block():
    A, B0, free, H = R.gs_scalar_case(32, "identity", False, 300)
    single, wide = _pair(H, {"AMGX_GSB_THREADS_MULTI": "1024"}, "hgs")
    lp = _float_level(single, "hybrid", wide=wide)
    assert lp["gs_block"] == 512 > A.shape[0] and lp["gs_threads"] == 1024
    _twin_operations(single, wide, free, 300, "partial block")


def test_twin_long_rows_fall_back_to_multicolour():
    """a longest row of 257 entries: the level keeps the multicolour form (G = 16) under sm_type "hgs" """
    A, B, free, H = R.gs_scalar_case(257, "identity")
    assert B == 0
    single, wide = _pair(H, {}, "hgs")
    lp = _float_level(single, "mc", wide=wide)
    assert lp["gs_lanes"] == 16 and lp["gs_split"] == 1
    _twin_operations(single, wide, free, 257, "257")


@pytest.mark.parametrize("rowrel", [False, True])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("G,L", [(1, 3), (2, 7), (4, 15), (8, 31), (16, 64)])
def test_twin_multicolour(G, L, l1, rowrel):
    """gs_color_kernel<G, float> and gs_upper_residual_kernel<G, float>: the split images (plain inverse diagonal) and the whole
    copy + the image of A (l1 inverse diagonal); AMGX_GS_ROWREL: row-relative 16-bit columns"""
    A = R.gs_scalar_case(L, "identity")[0]
    free = np.ones(A.shape[0], np.uint8)
    H = R.gs_hierarchy(A, free, l1_dinv=l1, seed=L)
    single, wide = _pair(H, {"AMGX_GS_ROWREL": "1"} if rowrel else {}, "gs")
    lp = _float_level(single, "mc", wide=wide)
    assert lp["gs_lanes"] == G and lp["gs_split"] == (0 if l1 else 1) and single.level_extra(0)["gs_rowrel"] == int(rowrel), lp
    _twin_operations(single, wide, free, G, (G, l1, rowrel))


# (tests/test_gpu_down_family.py: the Kuhn problem whose rest takes each form of the fused residual + restriction)
P3 = ((41, 37, 29), "right|top", 10)
ONE = {"AMGX_SELL_MAX_LANES": "1"}
DOWN_FORMS = {
    None: (_env(ONE, NO_DENSE, {"AMGX_NO_FUSED_RESTRICT": "1"}), 0),
    "sell": (_env(ONE, NO_DENSE, {"AMGX_NO_SELL_WINDOW": "1"}), 0),
    "sell-win": (_env(ONE, NO_DENSE), 0),
    "sell-lw": (_env(NO_DENSE, {"AMGX_LW_MIN_ROWS": "300"}), 1),
}


@pytest.mark.parametrize("form", list(DOWN_FORMS), ids=[str(k) for k in DOWN_FORMS])
def test_twin_residual_after_the_sweep_from_zero_in_every_form(form):
    """level_paths entry 33: c .* x - rest x as a product of its own (0), fused with the chunk-local restriction on sliced-ELL (1), on
    row windows (2) and on the local window (3)"""
    p, H = poisson_case(*P3)
    env, level = DOWN_FORMS[form]
    single, wide = _pair(H, env, "hgs")
    _float_level(single, "hybrid", 0, wide)
    lp = _float_level(single, "hybrid", level, wide)
    assert lp["gs_down"] == form and lp["gs_split"] == 1, lp
    assert "rest" in single.gs_prec_info(level)["images"] and (form != "sell-lw" or "restLW" in single.gs_prec_info(level)["images"])
    b = rhs(p, 1)
    want = _mult(wide, b)
    for device, graph in RUNS:
        assert np.array_equal(_mult(single, b, device, graph), want), (form, device, graph)
    assert not np.array_equal(want, _mult(_dev(H, env, sm_type="hgs"), b))
    SEEN_DOWN.add(form)


def test_every_residual_form_ran():
    """entry 33 took each of its four values in at least one twin case above (this file runs top to bottom)"""
    assert {None, "sell", "sell-win", "sell-lw"} <= SEEN_DOWN, SEEN_DOWN


# ---- 2. other cycles, the proxy smoother, SmoothVFromLevel ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(mg_cycle="W"), dict(mg_cycle="BS"), dict(sm_steps=2), dict(sm_symm=True)],
                         ids=["V", "W", "BS", "steps2", "symm"])
@pytest.mark.parametrize("sm", ["hgs", "gs"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_twin_cycles_and_the_proxy_smoother(grid, sm, kw):
    p, H = _grid(grid)
    key = tuple(sorted(kw.items()))
    single, wide = _handle(grid, sm, "single_gs_all", (), key), _handle(grid, sm, "wide", (), key)
    _float_level(single, "hybrid" if sm == "hgs" else "mc", wide=wide)
    assert single.cycle_info()["dense_level"] < 0
    _twin_operations(single, wide, np.asarray(p.free), 4, (grid, sm, kw), device_smooth=True)
    # SmoothVFromLevel: the sub-cycle from level 1 as a smoother
    n1 = single.sizes[1]
    x1, b1 = _inputs(H.levels[1].free, n1, 12)
    res = []
    for dev in (single, wide):
        x, r = x1.copy(), np.zeros(n1)
        dev.SmoothVFromLevel(1, x, b1, r, False, True, False)
        res.append((x, r))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (grid, sm, kw)


# ---- 3. without the split: a double handle on rounded levels, and the oracle ---------------------------------------------------------
def _rounded(H, single, lv):
    """RoundedHierarchy(H, lv) whose hybrid levels carry the smoother data the single handle was created with (from the TRUE A)"""
    import copy
    RH = RoundedHierarchy(H, lv)
    for i, info in enumerate(single.hgs):
        if info is not None:
            L = copy.copy(RH.levels[i])
            L.hgs_pre = dict(B=info["B"], color=info["color"], n_colors=info["n_colors"], dinv=info["dinv"])
            RH.levels[i] = L
    return RH


def _nosplit_case(name):
    if name in GRIDS:                                        # block-hybrid without the split
        p, H = _grid(name)
        return H, "hgs", _env(NO_DENSE, NO_SPLIT), "hybrid", [rhs(p, s) for s in (3, 8)]
    L = int(name[2:])                                        # multicolour with an l1 inverse diagonal: no split
    A = R.gs_scalar_case(L, "identity")[0]
    H = R.gs_hierarchy(A, np.ones(A.shape[0], np.uint8), l1_dinv=True, seed=L)
    rng = np.random.default_rng(L)
    return H, "gs", NO_DENSE, "mc", [rng.standard_normal(A.shape[0]) for _ in range(2)]


@pytest.mark.parametrize("name", list(GRIDS) + ["mc7", "mc31"])
def test_bitwise_against_a_double_handle_on_rounded_levels_and_the_oracle(name):
    """Oracle maxima measured on an MI355X (the print of every case): 2.3e-16 ... 3.5e-15 over the five cases (bound 1e-10)."""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    H, sm, env, form, B = _nosplit_case(name)
    # (images on level 0 only: the levels below may have the split images -- multicolour levels with a plain inverse diagonal --, or
    #  belong to the single-workgroup tail, whose copies stay fp64 and true)
    single = _dev(H, env, sm_type=sm, mat_prec=["single_gs_all"] + ["double"] * (H.n_levels - 1))
    lp = _float_level(single, form)
    assert lp["gs_split"] == 0
    lv = [l for l in range(single.n_levels) if single.gs_prec_info(l)["f32"]]
    assert lv == [0] and "A" in single.gs_prec_info(0)["images"], lv
    RH = _rounded(H, single, lv)
    assert not np.array_equal(np.asarray(RH.levels[0].A.val), np.asarray(H.levels[0].A.val)) and RH.levels[0].dinv is H.levels[0].dinv
    double = _dev(RH, env, sm_type=sm)
    assert all(double.gs_prec_info(l)["mask"] == 0 for l in range(double.n_levels))
    assert [double.level_paths(l) for l in range(H.n_levels)] == [single.level_paths(l) for l in range(H.n_levels)]
    for b in B:
        want = _mult(double, b)
        for device, graph in RUNS:
            got = _mult(single, b, device, graph)
            assert np.array_equal(got, want), (name, device, graph, _rel(got, want))
    # the sweeps read the float images; update_res outside pre-smoothing reads the TRUE A, as amgx_residual does
    n = single.sizes[0]
    x0, bb = _inputs(np.ones(n) if sm == "gs" else H.levels[0].free, n, 17)
    for back in (False, True):
        for xz in (False, True):
            xs, xd = (np.zeros_like(x0) if xz else x0.copy()), (np.zeros_like(x0) if xz else x0.copy())
            rs, rd, rt = np.zeros_like(bb), np.zeros_like(bb), np.zeros_like(bb)
            single.Smooth(0, xs, bb, rs, update_res=True, x_zero=xz, back=back)
            double.Smooth(0, xd, bb, rd, update_res=True, x_zero=xz, back=back)
            single.Residual(0, xs, bb, rt)
            assert np.array_equal(xs, xd) and np.array_equal(rs, rt), (name, back, xz)
    if sm == "gs":
        orc = Oracle(RH.levels, sm_type="gs_mc")
    else:
        olv, types = hgs_levels(RH.levels, single.hgs)
        orc = Oracle(olv, sm_type=types)
    worst = max(_rel(_mult(single, b), orc.apply(np.array(b))) for b in B)
    print(f"{name} {form}: vs oracle on rounded levels {worst:.2e} (1e-10)")
    assert worst <= 1e-10, (name, worst)


# ---- 4. the rounding is there, and small -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["V", "W", "BS"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_the_rounding_is_there_and_small(grid, cycle):
    """|Mult single - Mult double| / |Mult double| in [1e-10, 1.3e-6] for both orders, with and without the split.

    Measured on an MI355X (the prints below; smallest ... largest over block-hybrid, multicolour, block-hybrid without the split):
                    V                        W                        BS
        3d          2.90e-8 ... 4.28e-8      2.90e-8 ... 3.12e-8      2.93e-8 ... 2.99e-8
        2d          4.01e-8 ... 9.44e-8      5.02e-8 ... 5.20e-8      4.80e-8 ... 4.92e-8
        3d-odd      3.72e-8 ... 4.26e-8      3.63e-8 ... 3.79e-8      3.61e-8 ... 3.78e-8
    The W / BS figures rest on update_res reading the fp64 A outside pre-smoothing from zero (Handle::base_smooth)."""
    p, H = _grid(grid)
    b = rhs(p, 3)
    kw = () if cycle == "V" else (("mg_cycle", cycle),)
    lo, hi = np.inf, 0.0
    for sm, extra in (("hgs", ()), ("gs", ()), ("hgs", tuple(NO_SPLIT.items()))):
        single, double = _handle(grid, sm, "single_gs_all", extra, kw), _handle(grid, sm, "double", extra, kw)
        _float_level(single, "hybrid" if sm == "hgs" else "mc")
        assert all(double.gs_prec_info(l)["mask"] == 0 for l in range(double.n_levels))
        e = _rel(_mult(single, b), _mult(double, b))
        print(f"{grid} {sm} {dict(extra)} {cycle}: change {e:.2e}")
        lo, hi = min(lo, e), max(hi, e)
    print(f"{grid} {cycle}: change of one application {lo:.2e} ... {hi:.2e}")
    assert 1e-10 <= lo and hi <= CHANGE_MAX, (grid, cycle, lo, hi)


# ---- 5. PCG ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", ["hgs", "gs"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_pcg(grid, sm):
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = _grid(grid)
    single, double = _handle(grid, sm, "single_gs_all"), _handle(grid, sm, "double")
    _float_level(single, "hybrid" if sm == "hgs" else "mc")
    A = H.levels[0].A.to_scipy()
    free = np.asarray(p.free).astype(bool)
    b = rhs(p, 3)
    its, res = {}, {}
    for key, dev in (("single", single), ("double", double)):
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
        cg.Solve(b)
        its[key] = cg.iterations
        assert cg.errors[-1] <= 1e-8 * cg.errors[0], (grid, sm, key)
        cg = NativeCGSolver(dev, dev, tol=1e-12, maxsteps=100)
        x = np.asarray(cg.Solve(b))
        assert cg.errors[-1] <= 1e-12 * cg.errors[0], (grid, sm, key)
        res[key] = np.linalg.norm((b - A @ x)[free]) / np.linalg.norm(b)
    print(f"{grid} {sm}: iterations to 1e-8 single {its['single']} double {its['double']} | true residual at 1e-12 "
          f"single {res['single']:.2e} double {res['double']:.2e}")
    assert abs(its["single"] - its["double"]) <= 1, (grid, sm, its)
    assert res["single"] <= 10.0 * res["double"], (grid, sm, res)


# ---- 6. what stays fp64, the kill switch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", ["hgs", "gs"])
def test_operator_products_read_the_fp64_image(sm):
    p, H = _grid("3d")
    single, double = _handle("3d", sm, "single_gs_all"), _handle("3d", sm, "double")
    _float_level(single, "hybrid" if sm == "hgs" else "mc")
    for level in (0, 1):
        n = single.sizes[level]
        x, b = _inputs(H.levels[level].free, n, 21 + level)
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
            assert np.array_equal(u, v), (sm, level)
        assert _rel(out[0][0], H.levels[level].A.to_scipy() @ x) <= 1e-13, (sm, level)       # the TRUE A, not the rounded one (6e-8)


@pytest.mark.parametrize("extra", [(), tuple(NO_SPLIT.items())], ids=["split", "nosplit"])
@pytest.mark.parametrize("sm", ["hgs", "gs"])
def test_kill_switch_gives_the_double_handle(sm, extra):
    p, H = _grid("3d")
    on, double = _handle("3d", sm, "single_gs_all", extra), _handle("3d", sm, "double", extra)
    _float_level(on, "hybrid" if sm == "hgs" else "mc")
    b = rhs(p, 3)
    want = _mult(double, b)
    for more in (NO_F32, _env(NO_F32, WIDE)):
        off = _dev(H, _env(NO_DENSE, dict(extra), more), sm_type=sm, mat_prec="single_gs_all")
        assert all(off.gs_prec_info(l) == double.gs_prec_info(l) and off.gs_prec_info(l)["mask"] == 0 for l in range(H.n_levels))
        assert all(off.level_extra(l)["gs_f32_images"] == 0 for l in range(H.n_levels))
        for device, graph in RUNS:
            assert np.array_equal(_mult(off, b, device, graph), want), (sm, device, graph)
        x0, bb = _inputs(p.free, p.n, 23)
        for u, v in zip(_smooth_all(off, 0, x0, bb), _smooth_all(double, 0, x0, bb)):
            assert np.array_equal(u, v), sm
    assert not np.array_equal(_mult(on, b), want)
    # "single_gs" on a scalar hierarchy stays the double handle
    sgs = _dev(H, _env(NO_DENSE, dict(extra)), sm_type=sm, mat_prec="single_gs")
    assert all(sgs.gs_prec_info(l)["mask"] == 0 for l in range(H.n_levels)) and np.array_equal(_mult(sgs, b), want)


# ---- 7. memory -------------------------------------------------------------------------------------------------------------------------
def test_memory():
    """entry 3 (released) > entry 2 (added) on every level with split images -- asserted by _float_level in every case above, and
    here on every level of both orders --, and the handle takes less device memory than the double handle on the (24, 22, 20) grid"""
    import torch
    H = _grid("3d-odd")[1]

    def held(prec, sm):
        torch.cuda.synchronize()
        m0 = torch.cuda.mem_get_info(0)[0]
        dev = _dev(H, NO_DENSE, sm_type=sm, mat_prec=prec)
        torch.cuda.synchronize()
        return m0 - torch.cuda.mem_get_info(0)[0], dev

    for sm in ("hgs", "gs"):
        m32, single = held("single_gs_all", sm)
        m64, double = held("double", sm)
        _float_level(single, "hybrid" if sm == "hgs" else "mc")
        info = [single.gs_prec_info(l) for l in range(H.n_levels)]
        for l, v in enumerate(info):
            print(f"{sm} level {l}: {v['images']} released {v['released']} B, converted arrays {v['bytes']} B")
            if single.level_paths(l)["gs_split"] and v["mask"]:
                assert v["released"] > v["bytes"], (sm, l, v)
        assert info[-1]["mask"] == 0                                            # the coarsest level ignores the request
        rel, add = sum(v["released"] for v in info), sum(v["bytes"] for v in info)
        print(f"{sm}: released {rel} B, converted arrays {add} B, device memory single {m32} B, double {m64} B")
        assert rel > add, (sm, rel, add)
        assert m32 < m64, (sm, m32, m64)
        del single, double


# ---- 8. multi-vector calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", ["hgs", "gs"])
def test_a_single_precision_handle_is_not_fused(sm):
    p, H = _grid("3d")
    single, wide, double = _handle("3d", sm, "single_gs_all"), _handle("3d", sm, "wide"), _handle("3d", sm, "double")
    _float_level(single, "hybrid" if sm == "hgs" else "mc", wide=wide)
    B = np.ascontiguousarray(np.stack([rhs(p, j) for j in range(5)]))
    for dev in (single, wide):
        for k in (1, 2, 4, 5):
            for fuse in ("gs", "gs_block"):
                plan = dev.multi_plan(k, fuse=fuse)
                assert plan["fused"] == 0 and plan["groups"] == [1] * k, (sm, k, plan)
                assert "single-precision Gauss-Seidel images (level 0)" in plan["note"], plan
        for k, interleaved, fuse in ((2, False, "gs"), (5, True, "gs+down"), (4, False, "gs_block")):
            Bin = np.array(B[:k].T if interleaved else B[:k], order="C")
            X = np.full_like(Bin, np.nan)
            dev.MultMulti(Bin, X, interleaved=interleaved, fuse=fuse)
            X = X.T if interleaved else X
            for j in range(k):
                assert np.array_equal(X[j], _mult(dev, np.ascontiguousarray(B[j]))), (sm, k, j)
        # a column of SmoothMulti is Smooth, a column of DownMulti is the column loop's, bit for bit
        x0, bb = _inputs(p.free, p.n, 25)
        X, Bm = np.ascontiguousarray(np.stack([x0, 2 * x0, bb, x0 + bb])), np.ascontiguousarray(np.stack([bb, bb, x0, x0]))
        one = X.copy()
        for j in range(4):
            dev.Smooth(0, one[j], np.ascontiguousarray(Bm[j]), np.zeros_like(bb))
        dev.SmoothMulti(0, X, Bm, fuse="gs")
        assert np.array_equal(X, one), sm
        Xf, Cf = dev.DownMulti(0, Bm, fuse="gs+down")
        Xl, Cl = dev.DownMulti(0, Bm)
        assert np.array_equal(Xf, Xl) and np.array_equal(Cf, Cl), sm
        for j in range(4):
            x1, c1 = dev.DownMulti(0, np.ascontiguousarray(Bm[j:j + 1]))
            assert np.array_equal(x1[0], Xf[j]) and np.array_equal(c1[0], Cf[j]), (sm, j)
    for a, c in zip(single.DownMulti(0, Bm), wide.DownMulti(0, Bm)):
        assert np.array_equal(a, c), sm
    # the double handle stays fused
    plan = double.multi_plan(4, fuse="gs")
    assert plan["fused"] == 1 and plan["note"] == "" and plan["groups"] == [4], plan


# ---- 9. a mixed per-level list ---------------------------------------------------------------------------------------------------------
def test_mixed_per_level_list():
    p, H = _grid("3d")
    n = H.n_levels
    b = rhs(p, 3)
    double = _handle("3d", "hgs", "double")
    for prec, want in ((["single_gs_all", "double"] + ["single_gs_all"] * (n - 2), [0] + list(range(2, n - 1))),
                       (["double", "single_gs_all"] + ["double"] * (n - 2), [1])):
        single, wide = _dev(H, NO_DENSE, sm_type="hgs", mat_prec=prec), _dev(H, _env(NO_DENSE, WIDE), sm_type="hgs", mat_prec=prec)
        got = [l for l in range(n) if single.gs_prec_info(l)["f32"]]
        assert got == want and [l for l in range(n) if wide.gs_prec_info(l)["wide"]] == want, (prec, got)
        _float_level(single, "hybrid", want[0], wide)
        xs = _mult(single, b)
        assert np.array_equal(xs, _mult(wide, b)) and 1e-10 <= _rel(xs, _mult(double, b)) <= CHANGE_MAX, prec
    # Gauss-Seidel above a Chebyshev level: 2 on the one, 1 on the other
    types = ["hgs", "cheby"] + ["hgs"] * (n - 2)
    lm = [2.5] * n
    single = _dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm, mat_prec="single_gs_all")
    wide = _dev(H, _env(NO_DENSE, WIDE), sm_type=types, cheb_lambda_max=lm, mat_prec="single_gs_all")
    assert [bool(single.gs_prec_info(l)["f32"]) for l in range(n)] == [True, False] + [True] * (n - 3) + [False]
    _float_level(single, "hybrid", wide=wide)
    x = _mult(single, b)
    assert np.isfinite(x).all() and not np.array_equal(x, _mult(_dev(H, NO_DENSE, sm_type=types, cheb_lambda_max=lm), b))


# ---- 10. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_errors_and_queries():
    import dataclasses
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.device import hierarchy_desc
    from tests.problems import elasticity_case
    lib = _lib.hip()
    p, H = _grid("3d")
    n = H.n_levels
    pe, He = elasticity_case((7, 6, 5), False, 5)
    pb, Hb = elasticity_case((9, 8, 7), False, 5, 0.12)
    Hb.build_bgs()
    lm = [2.5] * n
    for hier, sm, kw, words in ((H, "jacobi", {}, ("Gauss-Seidel",)), (H, "cheby", dict(cheb_lambda_max=lm), ("Gauss-Seidel",)),
                                (Hb, "bgs", {}, ("Gauss-Seidel",)), (He, "hgs", {}, ("scalar",)), (He, "gs", {}, ("scalar",))):
        desc, keep, _ = hierarchy_desc(hier, sm_type=sm, **kw)
        desc.levels[0].mat_prec = _lib.AMGX_PREC_F32_SCALAR_GS
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, sm
        msg = lib.amgx_last_error(None).decode()
        assert "level 0" in msg and "mat_prec" in msg and all(w in msg for w in words), msg
    # AMGX_PREC_F32 stays an error on a scalar Gauss-Seidel level, 3 is no value
    for value, word in ((_lib.AMGX_PREC_F32, "mat_prec = AMGX_PREC_F32"), (3, "mat_prec must be")):
        desc, keep, _ = hierarchy_desc(H, sm_type="hgs")
        desc.levels[1].mat_prec = value
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, value
        msg = lib.amgx_last_error(None).decode()
        assert "level 1" in msg and word in msg, msg
    # a level with ghost columns, also through amgx_dist_create
    lv0 = H.levels[0]
    A = lv0.A
    ghost = RoundedHierarchy(H, [])
    ghost.levels[0] = dataclasses.replace(lv0, A=Matrix(A.n_rows, A.n_cols + 3, 1, 1, A.rowptr, A.col, A.val),
                                          dinv=np.concatenate([lv0.dinv, np.ones(3)]))
    desc, keep, _ = hierarchy_desc(ghost, sm_type="gs")
    desc.levels[0].mat_prec = _lib.AMGX_PREC_F32_SCALAR_GS
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0
    msg = lib.amgx_last_error(None).decode()
    assert "level 0" in msg and "mat_prec" in msg and "rank-partitioned" in msg, msg
    # the coarsest level ignores the value; every smoothed level takes it; the query and its bounds
    desc, keep, _ = hierarchy_desc(H, sm_type="hgs")
    for l in range(n):
        desc.levels[l].mat_prec = _lib.AMGX_PREC_F32_SCALAR_GS
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) == 0, lib.amgx_last_error(None).decode()
    out = np.full(8, -1, dtype=np.int64)
    ptr = out.ctypes.data_as(_lib.c_i64p)
    assert lib.amgx_gs_prec_info(h, 0, ptr, 8) == 0 and out[0] == 1 and out[1] & 2 and out[2] > 0 and out[3] > 0 and out[4] == 0, out
    assert list(out[5:]) == [-1, -1, -1]
    assert lib.amgx_gs_prec_info(h, n - 1, ptr, 5) == 0 and list(out[:5]) == [0, 0, 0, 0, 0]
    assert lib.amgx_gs_prec_info(h, n, ptr, 5) != 0 and lib.amgx_gs_prec_info(h, -1, ptr, 5) != 0 and lib.amgx_gs_prec_info(h, 0, ptr, 0) != 0
    assert "amgx_gs_prec_info" in lib.amgx_last_error(h).decode()
    ex = np.zeros(12, dtype=np.int64)
    assert lib.amgx_level_extra(h, 0, ex.ctypes.data_as(_lib.c_i64p), 12) == 0 and ex[9] == 1 and ex[10] >= 3 and ex[11] > 0, ex
    lib.amgx_destroy(h)
    # the only level of a single-level handle takes it (a stand-alone smoother)
    from ngsamg_amd import NgsAMG
    from tests.problems import to_matrix
    x0, bb = _inputs(p.free, p.n, 1)
    res = {}
    for prec, env in (("double", {}), ("single_gs_all", {}), ("wide", WIDE)):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            sm = NgsAMG.CreateHybridGSS(to_matrix(p), p.free, mat_prec="double" if prec == "double" else "single_gs_all")
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        x, r = x0.copy(), np.zeros(p.n)
        sm.Smooth(x, bb, r, False, True, False)
        res[prec] = (x, r)
    assert np.array_equal(res["single_gs_all"][0], res["wide"][0]) and np.array_equal(res["single_gs_all"][1], res["wide"][1])
    assert not np.array_equal(res["single_gs_all"][0], res["double"][0]) and _rel(res["single_gs_all"][0], res["double"][0]) <= 1e-6
    # a value beyond the range of float: the error names the level, for the float images and for the twin
    val = np.array(A.val, dtype=np.float64)
    val[7] = 1e39
    bad = RoundedHierarchy(H, [])
    bad.levels[0] = dataclasses.replace(lv0, A=Matrix(A.n_rows, A.n_cols, 1, 1, A.rowptr, A.col, val))
    for sm, extra in (("hgs", {}), ("gs", {}), ("hgs", NO_SPLIT)):
        for more in ({}, WIDE):
            with pytest.raises(_lib.NgsAMGError, match="single precision") as ei:
                _dev(bad, _env(NO_DENSE, extra, more), sm_type=sm, mat_prec="single_gs_all")
            assert "level 0" in str(ei.value), str(ei.value)
        _dev(bad, _env(NO_DENSE, extra, NO_F32), sm_type=sm, mat_prec="single_gs_all")       # ignored request: the double handle takes the matrix


def test_dist_create_refuses_the_value():
    """the C entry point of rank-partitioned hierarchies: refused before anything is built, naming level and field"""
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = _grid("3d")
    lib = _lib.hip()
    for sm, level in (("hgs", 0), ("gs", 1)):
        top, keep1, _ = hierarchy_desc(H, sm_type=sm, clev="none")
        top.levels[level].mat_prec = _lib.AMGX_PREC_F32_SCALAR_GS
        tail, keep2, _ = hierarchy_desc(H, sm_type=sm)
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
            msg = lib.amgx_comm_last_error(c).decode()
            assert f"level {level}" in msg and "mat_prec" in msg and "rank-partitioned" in msg, msg
        finally:
            lib.amgx_comm_destroy(c)


@pytest.mark.parametrize("sm", ["hgs"])
def test_time_op_of_the_sweeps(sm):
    """amgx_time_op ops 9 (the backward sweep inside whole cycles) and 5 (the down pass) run on the float images and leave a working
    handle behind"""
    import torch
    p, H = _grid("3d")
    b = torch.from_numpy(rhs(p, 6)).cuda()
    s = torch.cuda.Stream()                                                # (the probe needs a stream that is not the default one)
    with torch.cuda.stream(s):
        for prec in ("single_gs_all", "double"):
            dev = _dev(H, NO_DENSE, sm_type=sm, mat_prec=prec)
            if prec != "double":
                _float_level(dev, "hybrid")
            x0 = torch.empty_like(b); dev.Mult(b, x0)
            s.synchronize()
            for level in (0, 1):
                assert 0.0 < dev.time_op(level, 9, reps=2) < 50.0, (prec, level)
                assert 0.0 < dev.time_op(level, 5, reps=2) < 50.0, (prec, level)
            x1 = torch.empty_like(b); dev.Mult(b, x1)
            s.synchronize()
            assert torch.equal(x0, x1)
