"""Single-precision images for scalar Jacobi levels (jacobi_prec = "single", amgx_level_desc.jacobi_prec).

Definition under test: on a level that has the images (jacobi_prec_info(level)["f32"]) every value of A, A', the local-window image
of A', the symmetric diagonal image, Q and the local-window image of Q that the Jacobi passes of the level read is that image's stored
fp64 value rounded to float; index decode, gathers, LDS contents, accumulators and the order of additions are the fp64 kernels'.  Hence
  1. the handle equals, BIT FOR BIT, the "single_wide" handle (the fp64 kernels on fp64 images that hold the rounded values), in every
     selection below, through Mult (graph on / off, host / device pointers) and through the stage entry points of level 0;
  2. on the literal paths that have no A' / Q / diagonal image (sm_steps = 2, sm_symm: the ProxySmoother chains, AMGX_NO_FOLD=1) the
     V-cycle equals, bit for bit, a double handle on tests/mat_prec_ref.RoundedHierarchy; W / BS read the fp64 A in update_res of the
     second visit and are compared with the twin only;
  3. one application differs from the CPU emulation (tests/jacobi_prec_ref.py) and from the double handle by at most
     BOUND = 10 x 8.46e-8, the largest change the emulation shows against the double cycle over these problems (measured on the CPU,
     tests/test_jacobi_prec_cpu.py: 2.26e-8 ... 8.46e-8).  The emulation takes the form of every level from the handle: diagonal
     image, A' whose diagonal slot carries omega dinv_i (the own row's Dinv then comes from the rounded slot), plain A' (diagonal rounded), fp64 on
     the levels of the single-workgroup tail program.  The margin covers regrouped sums (1e-16) and float roundings that flip on the
     device's own Q and A' (formed on the device in another order of operations than scipy's);
  4. MatVec, Residual and the Krylov operator stay fp64: amgx_pcg to 1e-8 takes the double handle's iterations, a solve to 1e-12
     ends with a true residual of at most 10 x the double handle's;
  5. the interface: C-ABI errors name level and field, the coarsest level ignores the field, AMGX_NO_MAT_F32=1 gives the double handle,
     released bytes, the +-inf refusal, a mixed Jacobi / Chebyshev hierarchy, multi-vector calls stay the column loop.
Every case first asserts, through jacobi_prec_info and level_paths, that the image it names was converted and is the one the cycle runs.

Selections of level 0: the shapes of tests/test_gpu_dia_box.py with its BOX and OLD environments (box chunks / 512-row chunks of the
diagonal image), AMGX_NO_DIA=1 (sliced-ELL A'), AMGX_LW_MIN_ROWS=300 + AMGX_NO_DENSE_TAIL=1 (local-window images of A' and Q),
AMGX_NO_FOLD=1, mg_cycle W / BS, sm_steps = 2 / sm_symm (the literal passes on A)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests.jacobi_prec_ref import FoldedJacobiRef
from tests.mat_prec_ref import RoundedHierarchy
from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

# (shape, Dirichlet, max_coarse_size): tests/test_gpu_dia_box.py
PROBLEMS = [((6, 5, 70), "right|top", 10), ((9, 9, 9), "right|top", 10), ((7, 130), "left|top", 5), ((41, 37, 29), "right|top", 10)]
BIG = 3
BOX = {"AMGX_DIA_MIN_ROWS": "0", "AMGX_DIA_BOX_MIN_ROWS": "0", "AMGX_DIA_MAX_FILL": "1.5"}
OLD = dict(BOX, AMGX_NO_DIA_BOX="1")
NO_DIA = {"AMGX_NO_DIA": "1"}
LW = {"AMGX_LW_MIN_ROWS": "300", "AMGX_NO_DENSE_TAIL": "1"}
NO_FOLD = {"AMGX_NO_FOLD": "1"}
NO_F32 = {"AMGX_NO_MAT_F32": "1"}
# selection -> (environment, further arguments of DeviceAMGMatrix)
SEL = {
    "box": (BOX, ()), "old": (OLD, ()), "sell": (NO_DIA, ()), "lw": (LW, ()), "nofold": (dict(NO_DIA, **NO_FOLD), ()),
    "box-nofold": (dict(BOX, **NO_FOLD), ()), "W": (NO_DIA, (("mg_cycle", "W"),)), "BS": (NO_DIA, (("mg_cycle", "BS"),)),
    "box-W": (BOX, (("mg_cycle", "W"),)), "steps2": (NO_FOLD, (("sm_steps", 2),)), "symm": (NO_FOLD, (("sm_symm", True),)),
    "steps2-W": ({}, (("sm_steps", 2), ("mg_cycle", "W"))),
}
EVERY_SHAPE = ["box", "old", "sell", "nofold"]
BIG_ONLY = ["lw", "box-nofold", "W", "BS", "box-W", "steps2", "symm", "steps2-W"]
CASES = [(i, s) for i in range(len(PROBLEMS)) for s in EVERY_SHAPE] + [(BIG, s) for s in BIG_ONLY]
RUNS = ((False, True), (True, True), (True, False), (False, False))      # (device pointers, graph)
BOUND = 10 * 8.46e-8
BITS = {"A": 0, "Apre": 1, "ApreLW": 2, "dia": 3, "Q": 4, "QLW": 5}


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


def _case(i):
    shape, diri, mcs = PROBLEMS[i]
    return poisson_case(shape, diri, mcs)


@functools.lru_cache(maxsize=None)
def _handle(i, sel, prec):
    """one handle per (problem, selection, "single" | "single_wide" | "double"), shared by the tests"""
    env, kw = SEL[sel]
    return _dev(_case(i)[1], env, sm_type="jacobi", jacobi_prec=prec, **dict(kw))


def _b(i, seed=1):
    return rhs(_case(i)[0], seed)


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


def _images(dev, sel=None):
    """the levels whose passes read float images; with `sel`: level 0 (level 1 for "lw") has the image the selection names, converted,
    and it is the one the cycle runs"""
    lv = []
    for l in range(dev.n_levels - 1):
        i = dev.jacobi_prec_info(l)
        if i["f32"]:
            assert i["mask"] and i["bytes"] > 0 and not i["wide"], (l, i)
            lv.append(l)
    assert dev.jacobi_prec_info(dev.n_levels - 1)["mask"] == 0               # the coarsest level has no passes
    if sel is None:
        return lv
    assert lv and lv[0] == 0, (sel, lv)
    i0, lp = dev.jacobi_prec_info(0), dev.level_paths(0)
    if sel.startswith("box") or sel == "old":
        assert lp["kernel"] == "dia" and lp["compact"] == (0 if sel == "old" else 2) and "dia" in i0["images"] and "Apre" not in i0["images"], (sel, lp, i0)
    elif sel in ("sell", "nofold", "W", "BS"):
        assert lp["kernel"] == "sell" and "Apre" in i0["images"] and "dia" not in i0["images"], (sel, lp, i0)
        assert dev.matrix_info(0, "Apre")["fmt"] == "sell"
    elif sel == "lw":
        assert 1 in lv and dev.level_paths(1)["kernel"] == "sell-lw" and "ApreLW" in dev.jacobi_prec_info(1)["images"], (lv, dev.level_paths(1))
        assert any("QLW" in dev.jacobi_prec_info(l)["images"] and dev.matrix_info(l, "QLW")["fmt"] is not None for l in lv)
        assert dev.cycle_info()["dense_level"] < 0
    else:                                                                      # the ProxySmoother chains: A alone
        assert lp["kernel"] is None and i0["images"] == ("A",) and i0["released"] == 0, (sel, lp, i0)
    if "nofold" in sel or sel in ("W", "BS", "box-W", "steps2", "symm", "steps2-W"):
        assert not dev.is_folded(0) and "A" in i0["images"] and "Q" not in i0["images"], (sel, i0)
    else:
        # (Q in windowed sliced-ELL or CSR-vector form stays fp64 silently)
        assert dev.is_folded(0) and ("Q" in i0["images"] or "QLW" in i0["images"] or dev.matrix_info(0, "Q")["fmt"] in ("sellwin", "csrvec")), (sel, i0)
    assert dev.matrix_info(0, "A")["fmt"] == "sell" and "A" in i0["images"]
    return lv


def _forms(dev):
    """the form of every smoothed level for tests/jacobi_prec_ref.FoldedJacobiRef, read from the handle"""
    tail = dev.cycle_info()["tail_level"]
    forms = []
    for l in range(dev.n_levels - 1):
        info, lp, ex = dev.jacobi_prec_info(l), dev.level_paths(l), dev.level_extra(l)
        if (tail > 0 and l >= tail) or not info["f32"]:
            forms.append("double")                       # the tail program's CSR copies; a level without float images
        elif lp["kernel"] == "dia":
            forms.append("dia")
        elif ex["Apre_wdiag"] and lp["kernel"] != "sell-lw" and "Apre" in info["images"]:
            forms.append("apre_wd")
        else:
            forms.append("apre")
    return forms


# ---- 1. the twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,sel", CASES)
def test_single_equals_the_wide_twin_bit_for_bit(i, sel):
    single, wide, double = _handle(i, sel, "single"), _handle(i, sel, "single_wide"), _handle(i, sel, "double")
    lv = _images(single, sel)
    for l in range(single.n_levels):
        a, w, d = single.jacobi_prec_info(l), wide.jacobi_prec_info(l), double.jacobi_prec_info(l)
        assert w["f32"] == 0 and w["wide"] == (1 if l in lv else 0) and w["mask"] == a["mask"] and w["released"] == 0, (l, a, w)
        assert w["bytes"] == 2 * a["bytes"] and d == dict(d, f32=0, mask=0, bytes=0, released=0, wide=0), (l, a, w, d)
        assert single.level_paths(l) == wide.level_paths(l) == double.level_paths(l)
    b = _b(i)
    want = _mult(wide, b)
    assert np.all(np.isfinite(want))
    for device, graph in RUNS:
        assert np.array_equal(_mult(single, b, device, graph), want), (i, sel, device, graph)
        assert np.array_equal(_mult(wide, b, device, graph), want), (i, sel, device, graph)
    x64 = _mult(double, b)
    e = _rel(want, x64)
    print(f"{PROBLEMS[i][0]} {sel}: single against double {e:.2e}")
    assert 0 < e <= BOUND, (i, sel, e)


@pytest.mark.parametrize("i,sel", [(i, s) for i in range(len(PROBLEMS)) for s in ("box", "old", "sell")] + [(BIG, "lw"), (BIG, "nofold")])
def test_stage_entry_points_equal_the_twin(i, sel):
    single, wide = _handle(i, sel, "single"), _handle(i, sel, "single_wide")
    _images(single, sel)
    n0, n1 = single.sizes[0], single.sizes[1]
    b, xc = _b(i, 2), np.random.default_rng(3).standard_normal(n1)
    import torch
    out = {}
    for key, dev, on_device in (("single", single, False), ("wide", wide, False), ("single-device", single, True), ("wide-device", wide, True)):
        if on_device:
            give = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
            new = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            take = lambda t: t.cpu().numpy()
        else:
            give, new, take = (lambda v: v), (lambda n: np.full(n, np.nan)), (lambda v: v)
        x, r = new(n0), new(n0)
        dev.JacobiPre(0, give(b), x, r)
        xo = new(n0)
        dev.JacobiPost(0, give(_b(i, 4)), give(b), xo)
        res = [x, r, xo]
        if dev.is_folded(0):
            z, bc = new(n0), new(n1)
            dev.CycleDown(0, give(b), z, bc)
            up = z.clone() if on_device else np.array(z)
            dev.CycleUp(0, up, give(xc))
            res += [z, bc, up]
        if on_device:
            torch.cuda.synchronize()
        out[key] = [take(v) for v in res]
    assert all(len(v) == (3 if "nofold" in sel else 6) for v in out.values())
    for key in ("wide", "single-device", "wide-device"):
        for a, w in zip(out["single"], out[key]):
            assert np.all(np.isfinite(w)) and np.array_equal(a, w), (i, sel, key)


# ---- 2. the literal paths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["steps2", "symm"])
@pytest.mark.parametrize("i", [1, BIG])
def test_literal_v_cycle_is_the_double_cycle_on_the_rounded_matrix(i, sel):
    single = _handle(i, sel, "single")
    lv = _images(single, sel)
    assert all(single.jacobi_prec_info(l)["images"] == ("A",) for l in lv)
    env, kw = SEL[sel]
    rounded = _dev(RoundedHierarchy(_case(i)[1], lv), env, sm_type="jacobi", **dict(kw))
    b = _b(i)
    want = _mult(rounded, b)
    for device, graph in RUNS:
        assert np.array_equal(_mult(single, b, device, graph), want), (i, sel, device, graph)
    assert not np.array_equal(want, _mult(_handle(i, sel, "double"), b))


@pytest.mark.parametrize("i", [1, BIG])
def test_literal_passes_of_level_0_read_the_rounded_matrix(i):
    """amgx_jacobi_post (EP_JAC on A) and, on a level with a diagonal image, amgx_jacobi_pre (x = w Dinv b, r = b - A x on A):
    bit for bit the double handle's passes on the rounded level matrix"""
    single = _handle(i, "box", "single")
    _images(single, "box")
    rounded = _dev(RoundedHierarchy(_case(i)[1], [0]), NO_DIA, sm_type="jacobi")
    n0 = single.sizes[0]
    b, xin = _b(i, 2), _b(i, 4)
    got, want = np.full(n0, np.nan), np.full(n0, np.nan)
    single.JacobiPost(0, xin, b, got)
    rounded.JacobiPost(0, xin, b, want)
    assert np.array_equal(got, want)
    double = np.full(n0, np.nan)
    _handle(i, "box", "double").JacobiPost(0, xin, b, double)
    assert not np.array_equal(got, double)


# ---- 3. against the emulation and the double handle --------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["box", "old", "sell"])
@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_one_application_against_the_emulation(i, sel):
    """measured on an MI355X (printed below): against the emulation 3.9e-9 ... 3.6e-8, against the double handle 1.20e-8 ... 4.89e-8;
    on the CPU the emulation differs from the double cycle by 2.26e-8 ... 8.46e-8, BOUND = 10 x the largest"""
    single = _handle(i, sel, "single")
    _images(single, sel)
    H = _case(i)[1]
    forms = _forms(single)
    b = _b(i)
    x = _mult(single, b)
    e_ref = _rel(x, FoldedJacobiRef(H, forms=forms).apply(b))
    e_64 = _rel(x, _mult(_handle(i, sel, "double"), b))
    e_oracle = _rel(_mult(_handle(i, sel, "double"), b), FoldedJacobiRef(H, round32=False).apply(b))
    print(f"{PROBLEMS[i][0]} {sel}: forms {forms}")
    print(f"{PROBLEMS[i][0]} {sel}: against the emulation {e_ref:.2e}, against the double handle {e_64:.2e} (double handle against the fp64 emulation {e_oracle:.1e})")
    assert e_oracle <= 1e-12
    assert e_ref <= BOUND and e_64 <= BOUND, (i, sel, e_ref, e_64)


# ---- 4. the operator stays double ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["box", "sell"])
@pytest.mark.parametrize("i", range(len(PROBLEMS)))
def test_operator_and_krylov_stay_double(i, sel):
    from ngsamg_amd.krylov import NativeCGSolver
    p, H = _case(i)
    single, double = _handle(i, sel, "single"), _handle(i, sel, "double")
    _images(single, sel)
    n0 = single.sizes[0]
    x, b = _b(i, 5), _b(i, 6)
    for l in range(single.n_levels):
        n = single.sizes[l]
        xl, bl = np.random.default_rng(l).standard_normal(n), np.random.default_rng(10 + l).standard_normal(n)
        ys, yd, rs, rd = (np.full(n, np.nan) for _ in range(4))
        single.MatVec(l, xl, ys), double.MatVec(l, xl, yd)
        single.Residual(l, xl, bl, rs), double.Residual(l, xl, bl, rd)
        assert np.array_equal(ys, yd) and np.array_equal(rs, rd), l
    its = {}
    for key, dev in (("single", single), ("double", double)):
        cg = NativeCGSolver(dev, dev, tol=1e-8, maxsteps=100)
        cg.Solve(b)
        assert cg.errors[-1] <= 1e-8 * cg.errors[0]
        its[key] = cg.iterations
    A = H.levels[0].A.to_scipy()
    free = np.asarray(p.free).astype(bool)
    true = {}
    for key, dev in (("single", single), ("double", double)):
        cg = NativeCGSolver(dev, dev, tol=1e-12, maxsteps=200)
        xs = np.asarray(cg.Solve(b))
        assert cg.errors[-1] <= 1e-12 * cg.errors[0], (key, cg.iterations)
        true[key] = np.linalg.norm((b - A @ xs)[free]) / np.linalg.norm(b)
    print(f"{PROBLEMS[i][0]} {sel}: pcg 1e-8 iterations {its}, true residual after 1e-12 {true}")
    assert its["single"] == its["double"], (i, sel, its)
    assert true["single"] <= 10 * true["double"], (i, sel, true)
    assert x.size == n0


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_requests_and_the_coarsest_level_ignores_the_field():
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = _case(1)
    pe, He = elasticity_case((7, 6, 5), False, 5)
    lib = _lib.hip()
    n = H.n_levels
    cases = (
        (H, "cheby", 0, 1, ("level 0", "jacobi_prec", "Jacobi")), (H, "gs", 1, 2, ("level 1", "jacobi_prec", "Jacobi")),
        (H, "jacobi", 0, 3, ("level 0", "jacobi_prec", "got 3")), (H, "jacobi", 1, -1, ("level 1", "jacobi_prec", "got -1")),
        (He, "jacobi", 0, 1, ("level 0", "jacobi_prec", "block")),
    )
    for hier, sm, level, value, msgs in cases:
        desc, keep, _ = hierarchy_desc(hier, sm_type=sm)
        desc.levels[level].jacobi_prec = value
        h = C.c_void_p()
        assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0, (sm, level, value)
        msg = lib.amgx_last_error(None).decode()
        assert all(m in msg for m in msgs), msg
    # a level with ghost columns
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi")
    desc.levels[0].jacobi_prec = 1
    desc.levels[0].A.n_cols += 1
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0
    msg = lib.amgx_last_error(None).decode()
    assert "level 0" in msg and "jacobi_prec" in msg and "rank-partitioned" in msg, msg
    # mat_prec keeps its errors
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi", jacobi_prec="single")
    desc.levels[0].mat_prec = 1
    assert lib.amgx_create(C.byref(desc), C.byref(h)) != 0 and "mat_prec" in lib.amgx_last_error(None).decode()
    # the coarsest level ignores the field
    desc, keep, _ = hierarchy_desc(H, sm_type="jacobi")
    desc.levels[n - 1].jacobi_prec = 7
    h = C.c_void_p()
    assert lib.amgx_create(C.byref(desc), C.byref(h)) == 0, lib.amgx_last_error(None).decode()
    out = (C.c_int64 * 8)(*([-1] * 8))
    assert lib.amgx_jacobi_prec_info(h, n - 1, out, 8) == 0 and list(out) == [0, 0, 0, 0, 0, -1, -1, -1]
    assert lib.amgx_jacobi_prec_info(h, n, out, 5) != 0 and lib.amgx_jacobi_prec_info(h, 0, out, 0) != 0
    lib.amgx_destroy(h)
    # the entry counts of the other queries stay
    dev = _handle(1, "sell", "single")
    fmt, stored, lanes = C.c_int32(), C.c_int64(), C.c_int32()
    assert lib.amgx_matrix_info(dev._h, 0, 8, C.byref(fmt), C.byref(stored), C.byref(lanes)) != 0
    assert len(dev.level_extra(0)) == 12 and len(dev.level_paths(0)) == 40


def test_single_level_handle_takes_the_field():
    import ngsamg_amd.NgsAMG as N
    from tests.problems import to_matrix
    p, H = _case(BIG)
    out = {}
    for prec in ("single", "single_wide", "double"):
        sm = N.CreateJacobiSmoother(to_matrix(p), p.free, jacobi_prec=prec)
        dev = sm._amg._dev
        info = dev.jacobi_prec_info(0)
        assert info["images"] == (("A",) if prec != "double" else ()) and info["f32"] == (prec == "single"), (prec, info)
        x, b, r = _b(BIG, 7), _b(BIG, 8), np.full(p.n, np.nan)
        dev.Smooth(0, x, b, r, update_res=True)
        out[prec] = (x, r)
    assert np.array_equal(out["single"][0], out["single_wide"][0]) and np.array_equal(out["single"][1], out["single_wide"][1])
    assert not np.array_equal(out["single"][0], out["double"][0])


def test_kill_switch_gives_the_double_handle():
    for i, sel in ((1, "box"), (BIG, "sell")):
        env, kw = SEL[sel]
        off = _dev(_case(i)[1], dict(env, **NO_F32), sm_type="jacobi", jacobi_prec="single")
        for l in range(off.n_levels):
            info = off.jacobi_prec_info(l)
            assert info["f32"] == 0 and info["mask"] == 0 and info["bytes"] == 0 and info["released"] == 0, (l, info)
        b = _b(i)
        want = _mult(_handle(i, sel, "double"), b)
        for device, graph in RUNS:
            assert np.array_equal(_mult(off, b, device, graph), want), (i, sel, device, graph)
        assert not np.array_equal(_mult(_handle(i, sel, "single"), b), want)


def test_released_bytes_and_device_memory():
    """A level that has a float A' (or local-window A', or diagonal image) AND a float Q (or QLW) releases more fp64 bytes than its
    float arrays take, A's second array included: 8 (a' + q) > 4 (a + a' + q) with a' >= a stored entries, and on a diagonal-image
    level 8 (7 n + q) > 4 (a + 7 n + q) once Q stores more than 8 entries per row (13 here, 14.6 at cfg 2).  Asserted per level, for
    the whole handle, and on the device memory the handle takes against the double handle's -- for sliced-ELL A' and for the diagonal
    image with the local-window Q.  Exempt is exactly this: a level whose Q stays fp64 (windowed sliced-ELL or CSR-vector form, or an
    unfolded level).  There only half of A' or of the image is released against a whole float copy of A, and the level takes up to
    4 (a - 7 n) bytes more on a diagonal-image level; info[3] > 0 still holds on it."""
    import torch
    # (a problem of its own: the allocator hands out device memory in 2 MiB pieces, which hide the few MB of the other problems)
    H = poisson_case((61, 57, 53), "right|top", 10)[1]

    def held(prec, env):
        torch.cuda.synchronize()
        m0 = torch.cuda.mem_get_info(0)[0]
        dev = _dev(H, env, sm_type="jacobi", jacobi_prec=prec)
        torch.cuda.synchronize()
        return m0 - torch.cuda.mem_get_info(0)[0], dev

    for sel, env in (("sell", NO_DIA), ("box", dict(BOX, **LW))):
        m32, single = held("single", env)
        m64, double = held("double", env)
        lv = _images(single, sel)
        info = [single.jacobi_prec_info(l) for l in lv]
        for l, v in zip(lv, info):
            print(f"{sel} level {l}: {v['images']} released {v['released']} B, float arrays {v['bytes']} B")
            down = set(v["images"]) & {"Apre", "ApreLW", "dia"}
            up = set(v["images"]) & {"Q", "QLW"}
            if down or up:
                assert v["released"] > 0, (sel, l, v)
            if down and up:
                assert v["released"] > v["bytes"], (sel, l, v)
        assert set(info[0]["images"]) >= ({"A", "dia", "QLW"} if sel == "box" else {"A", "Apre"}) and set(info[0]["images"]) & {"Q", "QLW"}, info[0]
        rel, add = sum(v["released"] for v in info), sum(v["bytes"] for v in info)
        print(f"{sel}: released {rel} B, float arrays {add} B, device memory single {m32} B, double {m64} B")
        assert rel > add, (sel, rel, add)
        assert m32 < m64, (sel, m32, m64)
        del single, double
    # the exempt configuration: the diagonal image beside a Q that stays in windowed sliced-ELL / CSR-vector form
    for i in range(len(PROBLEMS)):
        dev = _handle(i, "box", "single")
        v = dev.jacobi_prec_info(0)
        if not set(v["images"]) & {"Q", "QLW"}:
            assert dev.matrix_info(0, "Q")["fmt"] in ("sellwin", "csrvec") and v["released"] > 0, (i, v)


def test_dist_create_refuses_the_field():
    """the C entry point of rank-partitioned hierarchies: refused before anything is built, naming level and field"""
    from ngsamg_amd import _lib
    from ngsamg_amd.device import hierarchy_desc
    p, H = _case(1)
    lib = _lib.hip()
    for level, value in ((0, 1), (1, 2)):
        top, keep1, _ = hierarchy_desc(H, sm_type="jacobi", clev="none")
        top.levels[level].jacobi_prec = value
        tail, keep2, _ = hierarchy_desc(H, sm_type="jacobi")
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
            assert f"level {level}" in msg and "jacobi_prec" in msg and "rank-partitioned" in msg, msg
        finally:
            lib.amgx_comm_destroy(c)


def test_values_beyond_single_precision_are_refused():
    import dataclasses
    from ngsamg_amd import _lib
    from ngsamg_amd._lib import Matrix
    p, H = _case(1)
    A = H.levels[0].A
    val = np.array(A.val, dtype=np.float64)
    val[7] = 1e39
    bad = RoundedHierarchy(H, [])
    bad.levels[0] = dataclasses.replace(H.levels[0], A=Matrix(A.n_rows, A.n_cols, A.br, A.bc, A.rowptr, A.col, val))
    for prec in ("single", "single_wide"):
        with pytest.raises(_lib.NgsAMGError, match="single precision") as ei:
            _dev(bad, sm_type="jacobi", jacobi_prec=prec)
        assert "level 0" in str(ei.value) and ("jacobi_prec = AMGX_JACOBI_PREC_F32_WIDE)" if prec == "single_wide" else "jacobi_prec = AMGX_JACOBI_PREC_F32)") in str(ei.value)
    _dev(bad, sm_type="jacobi")                                           # the double handle takes the matrix


def test_mixed_hierarchy_takes_both_options():
    p, H = _case(BIG)
    n = H.n_levels
    types = ["jacobi"] + ["cheby"] * (n - 1)
    b = _b(BIG)
    out = {}
    for prec in ("single", "single_wide", "double"):
        dev = _dev(H, dict(NO_DIA, AMGX_NO_DENSE_TAIL="1"), sm_type=types, mat_prec="single", jacobi_prec=prec, cheb_lambda_max=2.5)
        info = dev.jacobi_prec_info(0)
        assert (info["f32"], info["wide"]) == {"single": (1, 0), "single_wide": (0, 1), "double": (0, 0)}[prec], info
        assert all(dev.jacobi_prec_info(l)["mask"] == 0 for l in range(1, n))
        assert dev.matrix_info(0, "A32")["fmt"] == ("sell" if prec == "single" else None)
        assert any(dev.matrix_info(l, "A32")["fmt"] is not None for l in range(1, n - 1))      # the Chebyshev levels took mat_prec
        out[prec] = _mult(dev, b)
    assert np.array_equal(out["single"], out["single_wide"]) and not np.array_equal(out["single"], out["double"])
    assert _rel(out["single"], out["double"]) <= BOUND


@pytest.mark.parametrize("sel", ["box", "sell"])
def test_multi_vector_calls_stay_the_column_loop(sel):
    p, H = _case(BIG)
    single, wide = _handle(BIG, sel, "single"), _handle(BIG, sel, "single_wide")
    _images(single, sel)
    B = np.ascontiguousarray(np.stack([_b(BIG, j) for j in range(5)]))
    cols = [_mult(single, np.ascontiguousarray(B[j])) for j in range(5)]
    for fuse in (False, True, "gs", "gs_block", "down", "gs+down", "gs_block+down", "down_dia", "gs+down_dia", "gs_block+down_dia"):
        for dev in (single, wide):
            plan = dev.multi_plan(4, fuse)
            assert plan["fused"] == 0 and plan["groups"] == [1] * 4, (fuse, plan)
            assert "single-precision Jacobi images (level 0)" in plan["note"], (fuse, plan)
        for k in (2, 5):
            X = np.full_like(B[:k], np.nan)
            single.MultMulti(np.ascontiguousarray(B[:k]), X, fuse=fuse)
            for j in range(k):
                assert np.array_equal(X[j], cols[j]), (fuse, k, j)
    # the level-wise down pass keeps the column loop as well
    n1 = single.sizes[1]
    Xd, BC = single.DownMulti(0, np.ascontiguousarray(B[:4]), fuse="down_dia")
    z, bc = np.full(p.n, np.nan), np.full(n1, np.nan)
    single.CycleDown(0, np.ascontiguousarray(B[2]), z, bc)
    assert np.array_equal(Xd[2], z) and np.array_equal(BC[2], bc)
    assert _handle(BIG, sel, "double").multi_plan(4)["fused"] == 1


def test_time_ops_run_on_the_float_images():
    # (fresh handles: ops 8 needs the handle's own stream, which a call with device pointers replaces)
    single = _dev(_case(BIG)[1], BOX, sm_type="jacobi", jacobi_prec="single")
    _images(single, "box")
    for op in (1, 5, 6, 7, 8):
        assert single.time_op(0, op, reps=2) > 0, op
    lw = _dev(_case(BIG)[1], LW, sm_type="jacobi", jacobi_prec="single")
    _images(lw, "lw")
    for op in (5, 6, 8):
        assert lw.time_op(1, op, reps=2) > 0, op
