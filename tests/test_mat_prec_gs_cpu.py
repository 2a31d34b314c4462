"""Single-precision images for Gauss-Seidel on block levels (mat_prec = "single_gs") without a GPU: the vocabulary of
mat_prec, the flag path through Preconditioner, and the numerics of the definition on the CPU -- the oracle in the device's sweep
order on levels whose A.val went through float32 (tests/mat_prec_ref.rounded_levels) with the dinv of the TRUE A, against the same
oracle on the hierarchy; the Krylov operator is the fp64 A in both.

Bounds: the relative change of one application in [1e-9, 1e-6] (measured when the option was proposed: 3.4e-8 ... 6.1e-8 over the nine
shape / order pairs below; the lower end shows that the rounding is applied at all), PCG iterations to 1e-8 equal.

The environment switches of the option: AMGX_NO_MAT_F32=1 ignores every request, AMGX_GS_F32_WIDE=1 keeps fp64 images that hold the
rounded values (the A/B twin that tests/test_gpu_mat_prec_gs.py compares with, bit for bit)."""
import functools
import os

import numpy as np
import pytest

from tests.mat_prec_ref import pcg, rounded_levels
from tests.problems import elasticity_case, poisson_case, rhs, to_matrix

SHAPES = {"3d": ((14, 13, 12), False), "rot": ((12, 11, 10), True), "2d": ((40, 36), False)}


@functools.lru_cache(maxsize=None)
def case(shape):
    grid, rot = SHAPES[shape]
    return elasticity_case(grid, rot, 10)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- 1. the vocabulary ----------------------------------------------------------------------------------------------------
def test_single_gs_vocabulary():
    from ngsamg_amd import _lib
    from ngsamg_amd.device import mat_prec_levels
    E = _lib.NgsAMGError
    # scalar: the Chebyshev and the Gauss-Seidel smoothed levels, never the coarsest
    assert mat_prec_levels("single_gs", ["hgs"] * 4) == [1, 1, 1, 0]
    assert mat_prec_levels("single_gs", ["gs", "cheby", "jacobi", "gs"]) == [1, 1, 0, 0]
    assert mat_prec_levels("single_gs", ["hgs", "bgs", "cheby", "cheby"]) == [1, 0, 1, 0]
    assert mat_prec_levels("single_gs", ["gs"]) == [1]                                  # a stand-alone smoother is smoothed
    assert mat_prec_levels("single_gs", ["cheby"] * 3) == mat_prec_levels("single", ["cheby"] * 3) == [1, 1, 0]
    # "single" keeps its meaning: Chebyshev levels only
    assert mat_prec_levels("single", ["hgs", "cheby", "gs"]) == [0, 1, 0]
    assert mat_prec_levels("double", ["hgs"] * 3) == [0, 0, 0]
    # it needs at least one such level
    for types in (["jacobi"] * 3, ["bgs", "jacobi", "gs"], ["jacobi", "jacobi", "hgs"]):       # (gs on the coarsest only)
        with pytest.raises(E, match="single_gs.*no Chebyshev or Gauss-Seidel level"):
            mat_prec_levels("single_gs", types)
    with pytest.raises(E, match="no Chebyshev level"):
        mat_prec_levels("single", ["hgs"] * 3)
    # per-level lists: on those levels only, the coarsest ignores its entry
    assert mat_prec_levels(["single_gs", "double", "single_gs"], ["hgs", "hgs", "jacobi"]) == [1, 0, 0]
    assert mat_prec_levels(["single_gs", "single", "double", "double"], ["gs", "cheby", "jacobi", "gs"]) == [1, 1, 0, 0]
    assert mat_prec_levels(["double", "single_gs", "single_gs"], ["jacobi", "cheby", "bgs"]) == [0, 1, 0]
    for bad_type in ("jacobi", "bgs"):
        with pytest.raises(E, match="'single_gs' on level 1.*" + bad_type):
            mat_prec_levels(["double", "single_gs", "double"], ["hgs", bad_type, "hgs"])
    with pytest.raises(E, match="'single' on level 0.*Chebyshev"):
        mat_prec_levels(["single", "double"], ["hgs", "hgs"])
    with pytest.raises(E, match="one entry per level"):
        mat_prec_levels(["single_gs"], ["hgs", "hgs"])
    for bad in ("single-gs", "SINGLE_GS", "single_hgs", 2, None, ["single_gs", "half"]):
        with pytest.raises(E, match="unknown mat_prec"):
            mat_prec_levels(bad, ["hgs", "hgs"])


def test_descriptor_of_block_and_scalar_levels():
    """block Gauss-Seidel levels carry AMGX_PREC_F32; scalar ones have no sweep form with images and stay fp64 in the descriptor"""
    from ngsamg_amd.device import hierarchy_desc
    p, H = case("3d")
    n = H.n_levels
    for sm in ("hgs", "gs"):
        desc, keep, _ = hierarchy_desc(H, sm_type=sm, mat_prec="single_gs")
        assert [desc.levels[i].mat_prec for i in range(n)] == [1] * (n - 1) + [0], sm
        desc, keep, _ = hierarchy_desc(H, sm_type=sm)
        assert [desc.levels[i].mat_prec for i in range(n)] == [0] * n, sm
    types = ["hgs"] + ["cheby"] * (n - 1)
    desc, keep, _ = hierarchy_desc(H, sm_type=types, mat_prec="single_gs")
    assert [desc.levels[i].mat_prec for i in range(n)] == [1] * (n - 1) + [0]
    desc, keep, _ = hierarchy_desc(H, sm_type=types, mat_prec="single")
    assert [desc.levels[i].mat_prec for i in range(n)] == [0] + [1] * (n - 2) + [0]
    desc, keep, _ = hierarchy_desc(H, sm_type=types, mat_prec=["single_gs"] + ["double"] * (n - 1))
    assert [desc.levels[i].mat_prec for i in range(n)] == [1] + [0] * (n - 1)
    ps, Hs = poisson_case((33, 33), "left|top", 5)
    for sm in ("hgs", "gs"):
        desc, keep, _ = hierarchy_desc(Hs, sm_type=sm, mat_prec="single_gs")
        assert [desc.levels[i].mat_prec for i in range(Hs.n_levels)] == [0] * Hs.n_levels, sm
    tys = ["gs", "cheby"] + ["gs"] * (Hs.n_levels - 2)
    desc, keep, _ = hierarchy_desc(Hs, sm_type=tys, mat_prec="single_gs")
    assert [desc.levels[i].mat_prec for i in range(Hs.n_levels)] == [0, 1] + [0] * (Hs.n_levels - 2)


def test_preconditioner_flag_and_standalone_smoother():
    import inspect
    import ngsamg_amd.NgsAMG as N
    seen = {}

    class Probe:
        def __init__(self, hier, **kw):
            seen.clear()
            seen.update(kw, hier=hier)
            raise N.NgsAMGError("probe")

    p, H = elasticity_case((7, 6, 5), False, 5)
    old = N.DeviceAMGMatrix
    N.DeviceAMGMatrix = Probe
    try:
        for flags, want in ((dict(ngs_amg_sm_type="hgs", ngs_amg_mat_prec="single_gs"), "single_gs"),
                            (dict(ngs_amg_sm_type="gs", ngs_amg_mat_prec="Single_GS"), "single_gs"),
                            (dict(ngs_amg_sm_type="hgs"), "double")):
            with pytest.raises(N.NgsAMGError, match="probe"):
                N.Preconditioner(to_matrix(p), "ngs_amg.elast_3d", p.free, coords=p.coords, ngs_amg_max_coarse_size=5, **flags)
            assert seen["mat_prec"] == want, (flags, seen["mat_prec"])
        N.DeviceAMGMatrix = old
        # a request that cannot be met is refused before the library is loaded, naming what is missing
        with pytest.raises(N.NgsAMGError, match="single_gs.*no Chebyshev or Gauss-Seidel level"):
            N.Preconditioner(to_matrix(p), "ngs_amg.elast_3d", p.free, coords=p.coords, ngs_amg_max_coarse_size=5,
                             ngs_amg_sm_type="jacobi", ngs_amg_mat_prec="single_gs")
    finally:
        N.DeviceAMGMatrix = old
    assert inspect.signature(N.CreateHybridGSS).parameters["mat_prec"].default == "double"


def test_the_switches_and_the_abi_are_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "amgx.h")) as f:
        header = f.read()
    assert "AMGX_GS_F32_WIDE" in header and "AMGX_NO_MAT_F32" in header
    assert "#define AMGX_LEVEL_EXTRA_N 12" in header and "op = 11" in header
    assert "single-precision Gauss-Seidel images (level l)" in " ".join(header.split()).replace("* ", "")
    from ngsamg_amd.device import DeviceAMGMatrix
    assert DeviceAMGMatrix._EXTRA_KEYS[9:] == ("gs_f32", "gs_f32_images", "gs_f32_bytes") and len(DeviceAMGMatrix._EXTRA_KEYS) == 12


# ---- 2. the numerics of the definition --------------------------------------------------------------------------------------
ORDERS = {"hybrid-block": ("hgs", {}), "block-coloured": ("hgs", {"AMGX_BGSB_BC_MIN_ROWS": "0"}), "multicolour": ("gs", {})}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rounding_the_images_costs_nothing(shape, order):
    """the oracle in the device's sweep order; A.val of every smoothed level through float32, dinv that of the true A"""
    from ngsamg_amd.device import hierarchy_desc
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    p, H = case(shape)
    sm, env = ORDERS[order]
    smoothed = list(range(H.n_levels - 1))
    R = rounded_levels(H, smoothed)
    assert not np.array_equal(np.asarray(R[0].A.val), np.asarray(H.levels[0].A.val)) and R[0].dinv is H.levels[0].dinv
    if sm == "hgs":
        _, _, info = with_env(env, lambda: hierarchy_desc(H, sm_type="hgs"))       # blocks, colours and dinv of the TRUE A
        assert info[0] is not None and (info[0]["block_color"] is not None) == (order == "block-coloured")
        lv64, types = hgs_levels(H.levels, info)
        lv32, types32 = hgs_levels(R, info)
        assert types == types32 and types[0] == "gs_order"
    else:
        lv64, lv32, types = H.levels, R, "gs_mc"
    o64, o32 = Oracle(lv64, sm_type=types), Oracle(lv32, sm_type=types)
    b = rhs(p, 3)
    x64, x32 = o64.apply(np.array(b)), o32.apply(np.array(b))
    change = np.linalg.norm(x32 - x64) / np.linalg.norm(x64)
    A = H.levels[0].A.to_scipy()
    _, it64, e64 = pcg(o64, A, b, tol=1e-8, maxit=100)
    _, it32, e32 = pcg(o32, A, b, tol=1e-8, maxit=100)
    print(f"{shape} {order}: change {change:.2e} | pcg {it64} / {it32}")
    assert 1e-9 <= change <= 1e-6, (shape, order, change)
    assert it64 == it32, (shape, order, it64, it32)
    assert e32[-1] <= 1e-8 * e32[0] and e64[-1] <= 1e-8 * e64[0]
