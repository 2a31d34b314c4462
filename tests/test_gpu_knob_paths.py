"""The device paths behind environment switches (csrc/device/knobs.hpp) that no other test selects.

Every case builds its handle twice in one process -- with the environment as it is and with the switch set (the switches are read
by amgx_create) --, asserts through matrix_info / level_paths / level_extra / cycle_info that the switch changed the path it names
(AMGX_BSELL_XMODE: that the level is in the BSELL format, nothing reports the mode itself), and compares the results:

  * bit for bit with the default handle where the alternative keeps the order of the additions of every row (stated per test);
  * otherwise at the bound the suite already uses for the operation: 1e-12 against oracle.pyoracle.Oracle / cheby_ref.ChebyRef for
    Jacobi and Chebyshev cycles, 1e-10 for Gauss-Seidel cycles (gs_mc, tests.hgs_oracle), 1e-13 against scipy for a bare MatVec
    (test_gpu_kernel_zoo.py), 1e-13 between two launch forms of one cycle (test_gpu_dense_tail.py).

Right-hand sides by tests.problems.rhs, results pre-filled with NaN.  The measured maxima are printed."""
import functools

import numpy as np
import pytest

from ngsamg_amd._lib import Matrix, NgsAMGError
from tests.problems import elasticity_case, poisson_case, rhs
from tests.test_gpu_devbuild import env
from tests.test_gpu_kernel_zoo import _level, _rand_bcsr
from tests.test_gpu_kernel_zoo import _dev as _zoo_dev

pytestmark = pytest.mark.gpu

NO_DENSE = {"AMGX_NO_DENSE_TAIL": 1}
WHICH = ("A", "P", "PT", "Apre", "Q", "ApreLW", "QLW", "A32")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, e=None, **kw):
    from ngsamg_amd.device import DeviceAMGMatrix
    with env(**(e or {})):
        return DeviceAMGMatrix(H, device=0, **kw)


def _mult(d, b):
    x = np.full(b.size, np.nan)
    d.Mult(b, x)
    return x


def _smooth(d, level, x0, b, back=False, x_zero=False):
    x, r = x0.copy(), np.zeros(b.size)
    d.Smooth(level, x, b, r, False, False, x_zero, back=back)
    return x


def _report(d):
    """everything the handle reports about its paths, per level"""
    n = d.GetNLevels()
    return [({w: d.matrix_info(l, w) for w in WHICH}, d.level_paths(l), d.level_extra(l)) for l in range(n)], d.cycle_info()


def _level_vectors(d, level, seed):
    rng = np.random.default_rng(seed)
    n = d.sizes[level]
    return rng.standard_normal(n), rng.standard_normal(n)


# ---- a. AMGX_BSELL_XMODE ----------------------------------------------------------------------------------------------------

MODES = (1, 2, 3, 4, 5)
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 9)       # blocks per row, constant inside a slice: w < U, w = U and every w mod U for U = 2, 3, 4


@functools.lru_cache(maxsize=None)
def _xmode_level(bs):
    """one level of 39 whole slices of RB = 64 // bs block rows and a partial one; the rows of slice s hold WIDTHS[s % 8] blocks"""
    RB = 64 // bs
    n = 39 * RB + RB // 2 + 1
    rng = np.random.default_rng(bs)
    A = _rand_bcsr(rng, n, n, bs, bs, lambda i: WIDTHS[(i // RB) % len(WIDTHS)], 150)
    assert n % RB != 0 and sorted(set(np.diff(A.rowptr))) == sorted(WIDTHS)
    lev = _level(A)
    lev.dinv = np.ascontiguousarray(rng.standard_normal((n, bs, bs)).reshape(-1))
    return lev, A.to_scipy(), rng.standard_normal(n * bs), rng.standard_normal(n * bs)


def _xmode_dev(bs, mode):
    with env(AMGX_BSELL_XMODE=mode):
        dev = _zoo_dev([_xmode_level(bs)[0]])
    assert dev.matrix_info(0, "A")["fmt"] == "bsell", dev.matrix_info(0, "A")
    return dev


@pytest.mark.parametrize("bs", [2, 3, 6])
def test_bsell_xmode_synthetic_level(bs):
    """bsell_block_step<BS, true> (16-byte gathers), bsell_block_step_shfl (one load and a lane exchange) and
    bsell_row_dot_ahead<.., U> (column indices U blocks ahead) form the same products v * x and add them to the row's accumulator in
    the order of mode 0 -- block by block along the row, inside a block by pairs of columns -- so every mode gives the bits of mode 0
    on MatVec, Residual and JacobiPost; mode 0 against scipy at the bounds of test_block_matvec_and_jacobi."""
    lev, S, x, b = _xmode_level(bs)
    n = lev.A.n_rows
    out = {}
    for mode in (0,) + MODES:
        dev = _xmode_dev(bs, mode)
        y, r, xo = (np.full(n * bs, np.nan) for _ in range(3))
        dev.MatVec(0, x, y)
        dev.Residual(0, x, b, r)
        dev.JacobiPost(0, x, b, xo)
        out[mode] = (y, r, xo)
    y, r, xo = out[0]
    t = (b - S @ x).reshape(n, bs)
    ref = x + 0.9 * np.einsum("nij,nj->ni", lev.dinv.reshape(n, bs, bs), t).reshape(-1)
    print(f"bs {bs}: MatVec {_rel(y, S @ x):.2e}, Residual {_rel(r, b - S @ x):.2e}, JacobiPost {_rel(xo, ref):.2e}")
    assert _rel(y, S @ x) < 1e-13 and _rel(r, b - S @ x) < 1e-13 and _rel(xo, ref) < 1e-12
    for mode in MODES:
        for got, want, what in zip(out[mode], out[0], ("MatVec", "Residual", "JacobiPost")):
            assert np.array_equal(got, want), (bs, mode, what, _rel(got, want))


@pytest.mark.parametrize("bs", [2, 6])
def test_bsell_xmode_1_on_an_x_that_is_not_16_byte_aligned(bs):
    """mode 1 reads pairs of x with one 16-byte load only where x itself is 16-byte aligned (x16); a view that starts one double into
    a buffer is 8-byte aligned only and takes the 8-byte loads.  Same products in the same order: the bits of mode 0 both ways."""
    import torch
    lev, S, x, b = _xmode_level(bs)
    N = lev.A.n_rows * bs
    buf = torch.zeros(N + 4, dtype=torch.float64, device="cuda")
    got = {}
    for mode in (0, 1):
        dev = _xmode_dev(bs, mode)
        for off in (1, 2):
            xv = buf[off:off + N]
            assert xv.data_ptr() % 16 == (8 if off == 1 else 0)
            xv.copy_(torch.from_numpy(x))
            y = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
            dev.MatVec(0, xv, y)
            torch.cuda.synchronize()
            got[mode, off] = y.cpu().numpy()
    assert _rel(got[0, 2], S @ x) < 1e-13
    for key, v in got.items():
        assert np.array_equal(v, got[0, 2]), key


BLOCK_SHAPES = {"3d": ((14, 13, 12), False, 3), "rot": ((12, 11, 10), True, 6), "2d": ((40, 36), False, 2)}   # test_gpu_multi_gs_block.SHAPES
XMODE_CONFIGS = {
    "jacobi": ("jacobi", {}, None),
    "cheby": ("cheby", {}, None),
    "cheby-f32": ("cheby", {}, None),
    "hgs": ("hgs", {}, "hybrid-block"),
    "hgs-bc": ("hgs", {"AMGX_BGSB_BC_MIN_ROWS": 0}, "block-coloured"),
    "gs-bsell": ("gs", {"AMGX_BGS_BSELL_MIN": 1}, "mc-block-bsell"),
    "gs-bsell-nosplit": ("gs", {"AMGX_BGS_BSELL_MIN": 1, "AMGX_NO_BGS_SPLIT": 1}, "mc-block-bsell"),
}
_XREF = {}


@functools.lru_cache(maxsize=None)
def _cheb_lmax(shape):
    from tests.cheby_ref import power_estimate
    H = elasticity_case(BLOCK_SHAPES[shape][0], BLOCK_SHAPES[shape][1], 10)[1]
    return tuple([1.1 * power_estimate(lv, 20) for lv in H.levels[:-1]] + [1.0])


def _xmode_handle(shape, cfg, mode):
    sm, e, form = XMODE_CONFIGS[cfg]
    grid, rot, bs = BLOCK_SHAPES[shape]
    H = elasticity_case(grid, rot, 10)[1]
    kw = {}
    if sm == "cheby":
        kw = dict(cheb_lambda_max=list(_cheb_lmax(shape)), mat_prec="single" if cfg == "cheby-f32" else "double")
    d = _dev(H, dict(NO_DENSE, AMGX_BSELL_XMODE=mode, **e), sm_type=sm, **kw)
    assert H.levels[0].A.br == bs and d.matrix_info(0, "A")["fmt"] == "bsell" and d.cycle_info()["dense_level"] == -1
    assert d.level_paths(0)["gs_form"] == form, (shape, cfg, d.level_paths(0))
    if cfg == "cheby-f32":
        assert d.matrix_info(0, "A32")["fmt"] == "bsell"
    if cfg == "gs-bsell":
        assert d.level_paths(0)["gs_split"] == 1
    if cfg == "gs-bsell-nosplit":
        assert d.level_paths(0)["gs_split"] == 0
    return H, d


def _xmode_reference(shape, cfg, H, d, b):
    """the cycle of the reference on b: (result, bound); shared by the configurations that differ in the images only"""
    from oracle.pyoracle import Oracle
    sm = XMODE_CONFIGS[cfg][0]
    key = (shape, "gs" if sm == "gs" else cfg)
    if key not in _XREF:
        if sm == "jacobi":
            _XREF[key] = Oracle(H.levels, sm_type="jacobi").apply(b), 1e-12
        elif sm == "gs":
            _XREF[key] = Oracle(H.levels, sm_type="gs_mc").apply(b), 1e-10
        elif sm == "hgs":
            from tests.hgs_oracle import hgs_levels
            lv, types = hgs_levels(H.levels, d.hgs)
            _XREF[key] = Oracle(lv, sm_type=types).apply(b), 1e-10
        else:
            from tests.cheby_ref import ChebyRef
            RH = H
            if cfg == "cheby-f32":
                from tests.mat_prec_ref import RoundedHierarchy
                RH = RoundedHierarchy(H, [l for l in range(H.n_levels) if d.matrix_info(l, "A32")["fmt"] is not None])
            _XREF[key] = ChebyRef(RH, sm="cheby", degree=2, lambda_max=list(_cheb_lmax(shape)), cycle="V").apply(b), 1e-12
    return _XREF[key]


@pytest.mark.parametrize("cfg", list(XMODE_CONFIGS))
@pytest.mark.parametrize("shape", list(BLOCK_SHAPES))
def test_bsell_xmode_on_block_hierarchies(shape, cfg):
    """the BSELL kernels of a cycle -- bsell_spmv_kernel with every epilogue on the double and the float image (Jacobi, Chebyshev),
    bgs_bsell_color_kernel and bgs_bsell_upper_residual_kernel (gs with the BSELL copy, split or not) and bgsb_sweep_kernel (hgs,
    hybrid-block and block-coloured) -- take their row products through bsell.view(xmode): same products, same order (see
    test_bsell_xmode_synthetic_level), so Mult and a forward and a backward Smooth on level 0 give the bits of mode 0 in every
    mode.  Mode 0 against the reference of the smoother at the suite's bound."""
    p = elasticity_case(BLOCK_SHAPES[shape][0], BLOCK_SHAPES[shape][1], 10)[0]
    b = rhs(p, 4)
    H, d0 = _xmode_handle(shape, cfg, 0)
    ref, tol = _xmode_reference(shape, cfg, H, d0, b)
    x0 = _mult(d0, b)
    xs, bs_ = _level_vectors(d0, 0, 9)
    sm0 = [_smooth(d0, 0, xs, bs_, back) for back in (False, True)] + [_smooth(d0, 0, np.zeros(xs.size), bs_, False, True)]
    print(f"{shape} {cfg}: mode 0 vs reference {_rel(x0, ref):.2e} ({tol:g})")
    assert _rel(x0, ref) <= tol
    for mode in MODES:
        d = _xmode_handle(shape, cfg, mode)[1]
        assert np.array_equal(_mult(d, b), x0), (shape, cfg, mode)
        sm = [_smooth(d, 0, xs, bs_, back) for back in (False, True)] + [_smooth(d, 0, np.zeros(xs.size), bs_, False, True)]
        for got, want, what in zip(sm, sm0, ("forward", "backward", "forward from zero")):
            assert np.array_equal(got, want), (shape, cfg, mode, what)


def test_fused_multi_vector_cycle_ignores_the_xmode():
    """the multi-vector kernels have no xmode: MultMulti(fuse="gs_block") at k = 4 under mode 2 equals the same call under mode 0
    bit for bit, and Mult under mode 0 column by column at the bound between the fused cycle and Mult (1e-12, DESIGN.md 5.16: the
    fused cycle adds in another order than the single-vector one, so its columns are not the bits of Mult)"""
    p = elasticity_case(BLOCK_SHAPES["3d"][0], False, 10)[0]
    B = np.stack([rhs(p, 20 + j) for j in range(4)])
    H, d0 = _xmode_handle("3d", "hgs", 0)
    d2 = _xmode_handle("3d", "hgs", 2)[1]
    X0, X2 = np.full(B.shape, np.nan), np.full(B.shape, np.nan)
    d0.MultMulti(B, X0, fuse="gs_block")
    d2.MultMulti(B, X2, fuse="gs_block")
    assert d2.multi_plan(4, fuse="gs_block") == d0.multi_plan(4, fuse="gs_block")
    assert np.array_equal(X2, X0)
    worst = max(_rel(X2[j], _mult(d0, B[j])) for j in range(4))
    print(f"fused multi-vector cycle under mode 2 vs Mult under mode 0: {worst:.2e} (1e-12)")
    assert worst <= 1e-12


# ---- b. AMGX_GS_ROWREL ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,diri,mcs", [((17, 17, 17), "right|top", 20), ((33, 33), "left|top", 5)])
def test_gs_rowrel(shape, diri, mcs):
    """row-relative 16-bit columns in the colour-major SELL copies of multicolour Gauss-Seidel: sell_row_dot adds `row` (from the
    row list) to the decoded column and gathers the same x entries in the same order -- only the encoding differs, so cycle and
    sweeps give the bits of the default (absolute column bases).  Small levels sweep with several lanes per row
    (gs_color_kernel<G>) once the dense tail and the tail kernel are off."""
    from oracle.pyoracle import Oracle
    p, H = poisson_case(shape, diri, mcs)
    base = dict(NO_DENSE, AMGX_NO_TAIL_KERNEL=1)
    d0, d1 = _dev(H, base, sm_type="gs"), _dev(H, dict(base, AMGX_GS_ROWREL=1), sm_type="gs")
    levels = range(H.n_levels - 1)
    for d in (d0, d1):
        ci = d.cycle_info()
        assert ci["dense_level"] == -1 and ci["tail_level"] == -1
        assert all(d.level_paths(l)["gs_form"] == "mc" for l in levels)
    multi = [l for l in levels if d0.level_paths(l)["gs_lanes"] > 1]
    assert multi, [d0.level_paths(l)["gs_lanes"] for l in levels]
    e0, e1 = [d0.level_extra(l) for l in levels], [d1.level_extra(l) for l in levels]
    assert all(e["gs_rowrel"] == 0 for e in e0) and all(e["gs_rowrel"] == 1 for e in e1)
    assert all(e["gs_slices"] > 0 for e in e1) and sum(e["gs_slices16"] for e in e1) >= 1      # the 16-bit decode really runs
    assert any(e1[l]["gs_slices16"] >= 1 for l in multi)
    b = rhs(p, 3)
    x0, x1 = _mult(d0, b), _mult(d1, b)
    ref = Oracle(H.levels, sm_type="gs_mc").apply(b)
    print(f"{shape} gs: default vs oracle {_rel(x0, ref):.2e}, row-relative vs oracle {_rel(x1, ref):.2e} (1e-10)")
    assert _rel(x0, ref) <= 1e-10 and _rel(x1, ref) <= 1e-10
    assert np.array_equal(x1, x0)
    for l in sorted({0, multi[0], multi[-1]}):
        xs, bl = _level_vectors(d0, l, 5 + l)
        for back, zero in ((False, False), (True, False), (False, True)):
            s0 = _smooth(d0, l, np.zeros(xs.size) if zero else xs, bl, back, zero)
            s1 = _smooth(d1, l, np.zeros(xs.size) if zero else xs, bl, back, zero)
            assert np.array_equal(s1, s0), (l, back, zero)


# ---- c. AMGX_SELL_LONG_ROW_LANES --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _long_row_level(n):
    """n rows of 25 entries each (a window of 25 consecutive columns around the diagonal, clipped at the ends)"""
    rng = np.random.default_rng(n % 1000)
    start = np.clip(np.arange(n, dtype=np.int64) - 12, 0, n - 25)
    col = (start[:, None] + np.arange(25)[None, :]).astype(np.int32).reshape(-1)
    A = Matrix(n, n, 1, 1, np.arange(n + 1, dtype=np.int64) * 25, col, rng.standard_normal(col.size))
    return _level(A), A.to_scipy(), rng.standard_normal(n), rng.standard_normal(n)


@pytest.mark.parametrize("lanes", [2, 4])
def test_sell_long_row_lanes(lanes):
    """G lanes per row on a SELL image of rows of >= 24 entries.  The rule of upload_matrix only ever raises G (G = max(G, value)),
    and on a level of fewer than 2^20 / G rows it has grown G beyond the value already, so the smallest level the switch acts on has
    2^20 / 2 rows for 4 lanes (default: 2) and 2^20 rows for 2 lanes (default: 1).  Lanes per row change the order of the additions
    of a row: MatVec, JacobiPre and JacobiPost against scipy at the bounds of test_scalar_formats.  The device builder has its own
    copy of the rule (devbuild.hpp); AMGX_VERIFY_IMAGES=1 compares its image with the host's array by array."""
    n = (1 << 20) // 2 if lanes == 4 else 1 << 20
    lev, S, x, b = _long_row_level(n)
    d0 = _zoo_dev([lev])
    i0 = d0.matrix_info(0, "A")
    assert i0["fmt"] == "sell" and i0["lanes"] == lanes // 2, i0
    del d0
    for e in (dict(AMGX_SELL_LONG_ROW_LANES=lanes), dict(AMGX_SELL_LONG_ROW_LANES=lanes, AMGX_DEV_IMAGES_MIN_ROWS=0, AMGX_VERIFY_IMAGES=1)):
        with env(**e):
            dev = _zoo_dev([lev])
        info = dev.matrix_info(0, "A")
        assert info["fmt"] == "sell" and info["lanes"] == lanes, info
        y, xo, r, xp = (np.full(n, np.nan) for _ in range(4))
        dev.MatVec(0, x, y)
        dev.JacobiPre(0, b, xo, r)
        dev.JacobiPost(0, x, b, xp)
        errs = (_rel(y, S @ x), _rel(xo, 0.9 * b), _rel(r, b - S @ (0.9 * b)), _rel(xp, x + 0.9 * (b - S @ x)))
        print(f"{lanes} lanes, {n} rows: MatVec {errs[0]:.2e} (1e-13), JacobiPre {errs[1]:.2e} (1e-14) / {errs[2]:.2e} (1e-12), JacobiPost {errs[3]:.2e} (1e-12)")
        assert errs[0] < 1e-13 and errs[1] < 1e-14 and errs[2] < 1e-12 and errs[3] < 1e-12
        del dev


def test_lane_counts_outside_the_kernel_list_are_rounded_down():
    """AMGX_SELL_MAX_LANES=3 used to give G = 3 lanes per row (R = 64 / 3 rows per wave) although SELL kernels exist for 1, 2, 4, 8
    and 16 lanes only; Knobs::from_env rounds down, so the cap is 2 (the level of test_scalar_formats that takes 4 by default)"""
    n = 3000
    rng = np.random.default_rng(n + 20)
    A = _rand_bcsr(rng, n, n, 1, 1, lambda i: 20 + (i % 3) - 1, 100)
    S = A.to_scipy()
    x = rng.standard_normal(n)
    for e, lanes in (({}, 4), (dict(AMGX_SELL_MAX_LANES=3), 2), (dict(AMGX_SELL_MAX_LANES=7), 4), (dict(AMGX_SELL_LONG_ROW_LANES=3), 4)):
        with env(**e):
            dev = _zoo_dev([_level(A)])
        info = dev.matrix_info(0, "A")
        assert info["fmt"] == "sell" and info["lanes"] == lanes, (e, info)
        y = np.full(n, np.nan)
        dev.MatVec(0, x, y)
        assert _rel(y, S @ x) < 1e-13, (e, _rel(y, S @ x))


# ---- d. fallbacks of the Jacobi down pass and of Q --------------------------------------------------------------------------

LW_ENV = dict(NO_DENSE, AMGX_DEV_IMAGES_MIN_ROWS=0, AMGX_LW_MIN_ROWS=300)      # test_device_built_local_window_images_equal_host_built_ones
DOWN_CASES = (((26, 25, 24), "right|top", 20), ((9, 30, 13), ".*", 20), ((33, 33), "left|top", 5))


def _fused(lp):
    return lp["kernel"] is not None and lp["ept"] > 0


def _changed_qlw(d0, d1, n):
    return d0.matrix_info(0, "QLW")["fmt"] == "sell-lw" and all(d1.matrix_info(l, "QLW")["fmt"] is None for l in range(n))


def _changed_ept(d0, d1, n):
    on = [l for l in range(n) if _fused(d0.level_paths(l))]
    return bool(on) and not any(_fused(d1.level_paths(l)) for l in range(n))


def _changed_multi(d0, d1, n):
    on = [l for l in range(n) if _fused(d0.level_paths(l)) and d0.level_paths(l)["lanes"] > 1]
    one = [l for l in range(n) if _fused(d0.level_paths(l)) and d0.level_paths(l)["lanes"] == 1]
    return bool(on) and not any(_fused(d1.level_paths(l)) for l in on) and all(_fused(d1.level_paths(l)) for l in one)


def _changed_window(d0, d1, n):
    f0 = [(l, w) for l in range(n) for w in ("P", "PT", "Q") if d0.matrix_info(l, w)["fmt"] == "sellwin"]
    return any(d1.matrix_info(l, w)["fmt"] != "sellwin" for l, w in f0)


def _changed_diag_first(d0, d1, n):
    on = [l for l in range(n) if d0.level_extra(l)["A_diag_first"] or d0.level_extra(l)["Apre_diag_first"]]
    return bool(on) and not any(d1.level_extra(l)["A_diag_first"] or d1.level_extra(l)["Apre_diag_first"] for l in range(n))


# switch -> (environment of both handles, the switch, what must have changed)
DOWN_SWITCHES = {
    "AMGX_NO_QLW": (LW_ENV, {"AMGX_NO_QLW": 1}, _changed_qlw),
    "AMGX_FUSED_EPT_MAX": (LW_ENV, {"AMGX_FUSED_EPT_MAX": 0}, _changed_ept),
    "AMGX_NO_FUSED_RESTRICT_MULTI": (LW_ENV, {"AMGX_NO_FUSED_RESTRICT_MULTI": 1}, _changed_multi),
    "AMGX_NO_SELL_WINDOW_SHORT": (LW_ENV, {"AMGX_NO_SELL_WINDOW_SHORT": 1}, _changed_window),
    # (the diagonal comes first only in images with one lane per row: small levels have them under the lane cap)
    "AMGX_NO_DIAG_FIRST": (dict(LW_ENV, AMGX_SELL_MAX_LANES=1), {"AMGX_NO_DIAG_FIRST": 1}, _changed_diag_first),
}


@pytest.mark.parametrize("switch", list(DOWN_SWITCHES))
def test_jacobi_down_pass_fallbacks(switch):
    """AMGX_NO_QLW (Q without its local-window image), AMGX_FUSED_EPT_MAX=0 and AMGX_NO_FUSED_RESTRICT_MULTI (separate smoothing and
    restriction kernels, everywhere / on images with several lanes per row), AMGX_NO_SELL_WINDOW_SHORT (short ragged rows in the
    CSR-vector format instead of length-sorted windows) and AMGX_NO_DIAG_FIRST (CSR entry order; the Jacobi epilogues load the
    own-row value a second time).  All of them change the order of additions somewhere (another format, another kernel, the
    diagonal's position in the row), so: the Jacobi oracle at 1e-12 and the default handle at the 1e-13 bound between launch
    forms.  The first of DOWN_CASES whose default handle has the path is taken; a case list without one is a wrong list."""
    from oracle.pyoracle import Oracle
    base, sw, changed = DOWN_SWITCHES[switch]
    for shape, diri, mcs in DOWN_CASES:
        p, H = poisson_case(shape, diri, mcs)
        d0, d1 = _dev(H, base, sm_type="jacobi"), _dev(H, dict(base, **sw), sm_type="jacobi")
        if changed(d0, d1, H.n_levels):
            break
    else:
        pytest.fail(f"{switch}: no case of DOWN_CASES has the default path")
    b = rhs(p, 3)
    x0, x1 = _mult(d0, b), _mult(d1, b)
    ref = Oracle(H.levels, sm_type="jacobi").apply(b)
    print(f"{switch} on {shape}: default vs oracle {_rel(x0, ref):.2e}, switched vs oracle {_rel(x1, ref):.2e} (1e-12), mutual {_rel(x1, x0):.2e} (1e-13)")
    assert _rel(x0, ref) <= 1e-12 and _rel(x1, ref) <= 1e-12
    assert _rel(x1, x0) <= 1e-13
    if switch == "AMGX_NO_SELL_WINDOW_SHORT":
        # the transfers that lost their windows, on their own against scipy (the bound of test_transfer_block_shapes)
        rng = np.random.default_rng(1)
        moved = [(l, w) for l in range(H.n_levels - 1) for w in ("P", "PT")
                 if d0.matrix_info(l, w)["fmt"] == "sellwin" and d1.matrix_info(l, w)["fmt"] != "sellwin"]
        for l, w in moved:
            P = H.levels[l].P.to_scipy()
            xf, xc = rng.standard_normal(P.shape[0]), rng.standard_normal(P.shape[1])
            for d in (d0, d1):
                if w == "PT":
                    got = d.TransferF2C(l, xf, np.full(P.shape[1], np.nan))
                    assert _rel(got, P.T @ xf) <= 1e-13, (l, w, _rel(got, P.T @ xf))
                else:
                    got = d.AddC2F(l, -0.3, xf.copy(), xc)
                    assert _rel(got, xf - 0.3 * (P @ xc)) <= 1e-13, (l, w)
        print(f"AMGX_NO_SELL_WINDOW_SHORT: transfers without windows {moved}")


# ---- e. AMGX_GSB_NO_NARROW, AMGX_GSB_NO_MID ---------------------------------------------------------------------------------

@pytest.mark.parametrize("switch,key", [("AMGX_GSB_NO_NARROW", "gs_narrow"), ("AMGX_GSB_NO_MID", "gs_mid")])
def test_block_hybrid_sweep_takes_the_general_kernel(switch, key):
    """gsb_sweep_kernel<TH, G, FROM_ZERO, WP>: a lane holds WP pairs of entries and the odd trailing one of its slice in registers
    (narrow: WP = 2 for the sweep from zero, mid: WP = 5, general: WP = 8).  Whatever WP, the accumulations run over the pairs in
    their order, then over unused slots holding 0.0, then the trailing entry, followed by the same lane reduction -- a larger WP
    only adds zeros -- so the general kernel gives the bits of the narrow / mid-width one.  (33, 30, 28) is the case of
    test_gpu_multi_gs.py whose coarse levels take both."""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    p, H = poisson_case((33, 30, 28), "right|top", 20)
    d0, d1 = _dev(H, NO_DENSE, sm_type="hgs"), _dev(H, dict(NO_DENSE, **{switch: 1}), sm_type="hgs")
    levels = range(H.n_levels - 1)
    on = [l for l in levels if d0.level_paths(l)["gs_form"] == "hybrid" and d0.level_paths(l)[key] == 1]
    assert on, [d0.level_paths(l) for l in levels]
    assert all(d1.level_paths(l)[key] == 0 for l in levels)
    other = "gs_mid" if key == "gs_narrow" else "gs_narrow"
    assert [d1.level_paths(l)[other] for l in levels] == [d0.level_paths(l)[other] for l in levels]
    b = rhs(p, 3)
    x0, x1 = _mult(d0, b), _mult(d1, b)
    lv, types = hgs_levels(H.levels, d0.hgs)
    orc = Oracle(lv, sm_type=types)
    ref = orc.apply(b)
    print(f"{switch}: default vs oracle {_rel(x0, ref):.2e}, switched vs oracle {_rel(x1, ref):.2e} (1e-10); levels {on}")
    assert _rel(x0, ref) <= 1e-10 and _rel(x1, ref) <= 1e-10
    assert np.array_equal(x1, x0)
    for l in on:
        xs, bl = _level_vectors(d0, l, 11 + l)
        for back, zero in ((False, False), (True, False), (False, True)):
            xin = np.zeros(xs.size) if zero else xs
            s0, s1 = _smooth(d0, l, xin, bl, back, zero), _smooth(d1, l, xin, bl, back, zero)
            assert np.array_equal(s1, s0), (l, back, zero)
            xo, _ = orc.smooth(l, xin.copy(), bl, np.zeros(xs.size), False, False, zero, back)
            assert _rel(s1, xo) <= 1e-10, (l, back, zero, _rel(s1, xo))


# ---- f. AMGX_COARSE_DENSE_MAX -----------------------------------------------------------------------------------------------

def test_coarse_dense_max():
    """the refusal threshold of the device-side coarse inverse on the 40-unknown hierarchy of test_gpu_coarse_inverse.py: 39 refuses
    by name, 40 builds and solves within that file's residual bound"""
    from tests.test_gpu_coarse_inverse import _hierarchy
    H = _hierarchy(40)
    with pytest.raises(NgsAMGError, match="AMGX_COARSE_DENSE_MAX = 39"):
        _dev(H, dict(AMGX_COARSE_DENSE_MAX=39), sm_type="jacobi", clev="inv")
    dev = _dev(H, dict(AMGX_COARSE_DENSE_MAX=40), sm_type="jacobi", clev="inv")
    rng = np.random.default_rng(40)
    r = rng.standard_normal(40)
    xc = np.full(40, np.nan)
    dev.CoarseSolve(r, xc)
    er = np.linalg.norm(H.levels[-1].A.to_scipy() @ xc - r) / np.linalg.norm(r)
    print(f"AMGX_COARSE_DENSE_MAX=40: coarse solve residual {er:.2e} (1e-9)")
    assert er <= 1e-9


# ---- g. AMGX_SETUP_SERIAL, AMGX_SETUP_THREADS -------------------------------------------------------------------------------

@pytest.mark.parametrize("case,sm", [("poisson", "gs"), ("poisson", "jacobi"), ("elasticity", "hgs")])
def test_setup_threading_does_not_change_the_images(case, sm):
    """how the host builders of amgx_create are threaded (par_for, SetupTasks) must not show in what they build: every report of the
    handle equals the default's and Mult gives the same bits -- serial tasks, one builder thread, three (which does not divide the
    slice counts), and three with the device builders verified against the host's (AMGX_VERIFY_IMAGES=1 raises on a difference).
    Nothing reports the thread count itself; what is asserted is that it does not matter."""
    p, H = poisson_case((17, 17, 17)) if case == "poisson" else elasticity_case((9, 8, 7))
    b = rhs(p, 3)
    d0 = _dev(H, NO_DENSE, sm_type=sm)
    want, x0 = _report(d0), _mult(d0, b)
    assert np.isfinite(x0).all()
    for e in (dict(AMGX_SETUP_SERIAL=1), dict(AMGX_SETUP_THREADS=1), dict(AMGX_SETUP_THREADS=3), dict(AMGX_SETUP_SERIAL=1, AMGX_SETUP_THREADS=3)):
        d = _dev(H, dict(NO_DENSE, **e), sm_type=sm)
        assert _report(d) == want, e
        assert np.array_equal(_mult(d, b), x0), e
    dv0 = _dev(H, dict(NO_DENSE, AMGX_DEV_IMAGES_MIN_ROWS=0), sm_type=sm)
    dv = _dev(H, dict(NO_DENSE, AMGX_DEV_IMAGES_MIN_ROWS=0, AMGX_SETUP_THREADS=3, AMGX_VERIFY_IMAGES=1), sm_type=sm)
    assert _report(dv) == _report(dv0)
    assert np.array_equal(_mult(dv, b), _mult(dv0, b))


# ---- h. rank-partitioned handles: AMGX_DIST_EVENTS, AMGX_DIST_TAIL_GRAPH ----------------------------------------------------

DIST_VARIANTS = {
    "events-direct": dict(AMGX_DIST_EVENTS=1, AMGX_DIST_GRAPH=0),      # only direct launches are ordered by the event form
    "events-graph": dict(AMGX_DIST_EVENTS=1),
    "tail-graph-direct": dict(AMGX_DIST_TAIL_GRAPH=1, AMGX_DIST_GRAPH=0),
}


@pytest.mark.parametrize("variant", list(DIST_VARIANTS))
@pytest.mark.parametrize("sm", ["jacobi", "hgs"])
@pytest.mark.parametrize("R,box,dmin", [(2, (14, 12, 12), 100), (4, (10, 10, 10), 50)])
def test_rank_partitioned_stream_ordering_and_tail_graph(R, box, dmin, sm, variant):
    """virtual ranks on one GPU (LoopbackComm): cross-stream ordering by events instead of device flags, in direct launches and
    under the whole-cycle graph, and a graph of its own for the replicated tail between direct launches.  None of them touches a
    kernel or its arguments, so two applications give the bits of the default handle; the serial oracle on the assembled global
    hierarchy at 1e-12 (Jacobi) / 1e-10 (block-hybrid Gauss-Seidel)."""
    import torch
    from ngsamg_amd import dist as D
    from oracle.pyoracle import Oracle
    from tests.dist_oracle import oracle_bgs, oracle_sm_types
    pg = D.proc_grid(R, 3)

    def build(e):
        with env(**e):
            return D.DistributedAMG(D.LoopbackComm(R), [D.assemble_poisson_owned(r, pg, box) for r in range(R)], dim=3, dist_min_rows=dmin,
                                    device=0, max_coarse_size=10, sm_type=sm, **({"hgs_block_rows": 256} if sm == "hgs" else {}))
    e = DIST_VARIANTS[variant]
    a0, a1 = build({}), build(e)
    sts = a0.dist_levels[0]
    rng = np.random.default_rng(3)
    bh = [rng.standard_normal(s.n) * s.free for s in sts]
    bs = [torch.from_numpy(v).cuda() for v in bh]
    out = []
    for a in (a0, a1):
        xs = [torch.full((s.n,), float("nan"), dtype=torch.float64, device="cuda") for s in sts]
        first = None
        for rep in range(2):
            a.Mult(bs, xs)
            torch.cuda.synchronize()
            got = np.concatenate([x.cpu().numpy() for x in xs])
            if rep == 0:
                first = got
        assert np.array_equal(got, first)
        out.append(got)
    # the paths
    assert a0._dev.order_info() == "flags" and a0._dev.graph_info()["enabled"]
    assert all(o.tail.level_extra(0)["graphs"] == 0 for o in a0._dev.ops)
    assert a1._dev.order_info() == ("events" if "AMGX_DIST_EVENTS" in e else "flags")
    gi = a1._dev.graph_info()
    assert gi["enabled"] == ("AMGX_DIST_GRAPH" not in e) and (gi["replays"] >= 1) == ("AMGX_DIST_GRAPH" not in e), gi
    tail_graphs = [o.tail.level_extra(0)["graphs"] for o in a1._dev.ops]
    assert all(g >= 1 for g in tail_graphs) if "AMGX_DIST_TAIL_GRAPH" in e else all(g == 0 for g in tail_graphs), tail_graphs
    glv = a0.global_levels()
    ref = Oracle(glv, sm_type=oracle_sm_types(a0), bgs=oracle_bgs(a0, glv)).apply(np.concatenate(bh))
    tol = 1e-12 if sm == "jacobi" else 1e-10
    print(f"R = {R} {sm} {variant}: default vs oracle {_rel(out[0], ref):.2e}, switched vs oracle {_rel(out[1], ref):.2e} ({tol:g})")
    assert _rel(out[0], ref) <= tol and _rel(out[1], ref) <= tol
    assert np.array_equal(out[1], out[0])
