"""Device formats on reordered and non-Kuhn level matrices (tests/reorder.py).  amgx_create picks the format of every level from
the structure of its matrix; a matrix in a mesh generator's vertex order, or one that is not a Kuhn P1 matrix, takes branches the
natural-order problems never reach.  Every test asserts through DeviceAMGMatrix.level_paths (amgx_level_paths) that its target
path ran:

  path                                                   test
  32-bit slices on level 0 (fused down kernel)           test_level0_32bit_slices_and_chunks_with_more_slots_than_threads
  chunks with more slots than threads                    test_level0_32bit_slices_and_chunks_with_more_slots_than_threads
  DIA image with K = 1 .. 7, reversed Kuhn ordering      test_dia_k_matches_oracle_and_sell_path, test_dia_reversed_kuhn_and_refused_orderings
  DIA with 6 entries of P per thread                     test_ept6_dia
  SELL, 6 entries of P per thread, blocks 256/512/1024   test_ept6_sell_fused_block
  windowed image, 6 entries of P per thread              test_ept6_windowed_image
  G = 2 / 4 / 8 lanes per row, narrow and wide P         test_multi_lane_fused_restriction_with_wide_p
  local-window chunks over capacity                      test_local_window_chunks_without_window
  XCD workgroup placement (SELL, DIA, hgs)               test_xcd_placement_is_bit_identical*
  compact chunks                                         test_equivariance_jacobi (forced thresholds), test_gpu_dia, test_gpu_parity
"""
import numpy as np
import pytest

from tests import reorder as R
from tests.problems import elasticity_case, poisson_case, rhs

pytestmark = pytest.mark.gpu

# thresholds lowered so that the small problems take the big-level paths
FORCED = (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_COMPACT_CHUNKS_MIN_ROWS", "0"), ("AMGX_LW_MIN_ROWS", "300"), ("AMGX_SELL_MAX_LANES", "1"))
PROBLEMS = {"p3": lambda: poisson_case((41, 37, 29), "right|top", 10), "p2": lambda: poisson_case((130, 110), "left|top", 5),
            "e3": lambda: elasticity_case((9, 8, 7)), "e6": lambda: elasticity_case((9, 8, 7), rotations=True)}


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(H, monkeypatch, env=(), sm_type="jacobi", **kw):
    from ngsamg_amd.device import DeviceAMGMatrix
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type=sm_type, **kw)


def _apply(dev, b):
    x = np.full(b.size, np.nan)
    dev.Mult(b, x)
    return x


def _paths(dev):
    return [dev.level_paths(l) for l in range(dev.GetNLevels())]


_BASE = {}


def _base(name, env_name, cycle, monkeypatch):
    """dev(H) on the natural order, once per (problem, thresholds, cycle)"""
    key = (name, env_name, cycle)
    if key not in _BASE:
        p, H = PROBLEMS[name]()
        b = rhs(p, 1)
        _BASE[key] = _apply(_dev(H, monkeypatch, FORCED if env_name == "forced" else (), mg_cycle=cycle), b)
    return _BASE[key]


@pytest.mark.parametrize("env_name", ["forced", "default"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_equivariance_jacobi(name, kind, env_name, monkeypatch):
    """dev(Pi H Pi^T) = Pi_0 dev(H) = Oracle(Pi H Pi^T) for the Jacobi V / W / BS cycles"""
    from oracle.pyoracle import Oracle
    p, H = PROBLEMS[name]()
    perms = R.level_perms(H, kind, seed=7)
    Hp = R.permute_hierarchy(H, perms)
    b = rhs(p, 1)
    bp = R.permute_vec(b, perms[0], p.bs)
    env = FORCED if env_name == "forced" else ()
    for cycle in ("V", "W", "BS"):
        dev = _dev(Hp, monkeypatch, env, mg_cycle=cycle)
        x = _apply(dev, bp)
        assert _rel(x, R.permute_vec(_base(name, env_name, cycle, monkeypatch), perms[0], p.bs)) < 1e-12, cycle
        assert _rel(x, Oracle(Hp.levels, sm_type="jacobi", cycle=cycle).apply(bp)) < 1e-12, cycle
    if env_name == "forced" and p.bs == 1 and kind != "reverse":
        # scalar level 0 with forced thresholds: compact chunks of the SELL image (the DIA detector refuses these orderings;
        # identity and coarse_only keep the Kuhn diagonals)
        lp = dev.level_paths(0)
        assert lp["compact"] == 1 and lp["kernel"] == ("dia" if kind in ("identity", "coarse_only") else "sell")


@pytest.mark.parametrize("kind", ["reverse", "random", "rcm", "coarse_only"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_order_dependent_smoothers_on_reordered_hierarchy(name, kind, monkeypatch):
    """multicolour Gauss-Seidel, the block-hybrid form (hgs) and block Gauss-Seidel on the aggregates (bgs, block levels) of the
    reordered hierarchy against the oracle on the same hierarchy"""
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    p, H = PROBLEMS[name]()
    if p.bs > 1:
        H.build_bgs()
    Hp = R.permute_hierarchy(H, R.level_perms(H, kind, seed=11))
    Hp.options = getattr(H, "options", None)
    b = R.permute_vec(rhs(p, 2), R.level_perms(H, kind, seed=11)[0], p.bs)
    x = _apply(_dev(Hp, monkeypatch, sm_type="gs"), b)
    assert _rel(x, Oracle(Hp.levels, sm_type="gs_mc").apply(b)) < 1e-10
    dev = _dev(Hp, monkeypatch, sm_type="hgs")
    lv, types = hgs_levels(Hp.levels, dev.hgs)
    assert _rel(_apply(dev, b), Oracle(lv, sm_type=types).apply(b)) < 1e-10
    if p.bs > 1:
        bgs = [lv.bgs for lv in Hp.levels]
        assert all(g is not None for g in bgs[:-1])
        x = _apply(_dev(Hp, monkeypatch, sm_type="bgs"), b)
        assert _rel(x, Oracle(Hp.levels, sm_type="bgs_mc", bgs=bgs).apply(b)) < 1e-10


@pytest.mark.parametrize("kind", ["random", "rcm", "coarse_only", "slice64"])
@pytest.mark.parametrize("name", ["p3", "p2"])
def test_device_images_equal_host_images_on_reordered_levels(name, kind, monkeypatch):
    """AMGX_VERIFY_IMAGES compares every device-built image with the host builder bit for bit; host-built images give the same
    result bit for bit"""
    p, H = PROBLEMS[name]()
    perms = R.level_perms(H, kind, seed=5)
    Hp = R.permute_hierarchy(H, perms)
    b = R.permute_vec(rhs(p, 3), perms[0])
    small = FORCED + (("AMGX_DEV_IMAGES_MIN_ROWS", "0"),)
    xv = _apply(_dev(Hp, monkeypatch, small + (("AMGX_VERIFY_IMAGES", "1"),)), b)
    xd = _apply(_dev(Hp, monkeypatch, small), b)
    xh = _apply(_dev(Hp, monkeypatch, FORCED + (("AMGX_HOST_IMAGES", "1"),)), b)
    assert np.array_equal(xv, xd) and np.array_equal(xv, xh)


def test_reordered_fine_matrix_through_the_whole_pipeline(monkeypatch):
    """a fine matrix in a random vertex order (matrix, coordinates and free dofs permuted) through the host setup: every smoother
    against the oracle, and the device Galerkin hook gives the same hierarchy bit for bit"""
    from ngsamg_amd import _lib, fem
    from ngsamg_amd._lib import Matrix
    from ngsamg_amd.hierarchy import Hierarchy
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    f = fem.poisson_fast((30, 28, 26), dirichlet="right|top")
    perm = R.permutation("random", f.n, seed=3)
    A = R.permute_matrix(Matrix(f.n, f.n, 1, 1, f.rowptr, f.col, f.val), perm, perm)
    free, coords = np.asarray(f.free)[perm], np.asarray(f.coords).reshape(f.n, -1)[perm]
    kw = dict(dim=3, energy=0, max_coarse_size=50)
    try:
        assert _lib.device_setup(False) is False
        H0 = Hierarchy(A, free, coords, **kw)
        assert _lib.device_setup(True, min_rows=0) is True
        H1 = Hierarchy(A, free, coords, **kw)
    finally:
        _lib._device_setup = None
        _lib.device_setup()
    assert len(H0.levels) == len(H1.levels) >= 3
    for a, c in zip(H0.levels, H1.levels):
        for m0, m1 in ((a.A, c.A), (a.P, c.P)):
            if m0 is None:
                continue
            assert np.array_equal(m0.rowptr, m1.rowptr) and np.array_equal(m0.col, m1.col)
            assert np.array_equal(np.asarray(m0.val).view(np.uint64), np.asarray(m1.val).view(np.uint64))
    rng = np.random.default_rng(4)
    b = rng.standard_normal(f.n) * free
    assert _rel(_apply(_dev(H0, monkeypatch, FORCED), b), Oracle(H0.levels, sm_type="jacobi").apply(b)) < 1e-12
    assert _rel(_apply(_dev(H0, monkeypatch, sm_type="gs"), b), Oracle(H0.levels, sm_type="gs_mc").apply(b)) < 1e-10
    dev = _dev(H0, monkeypatch, sm_type="hgs")
    lv, types = hgs_levels(H0.levels, dev.hgs)
    assert _rel(_apply(dev, b), Oracle(lv, sm_type=types).apply(b)) < 1e-10


def test_level0_32bit_slices_and_chunks_with_more_slots_than_threads(monkeypatch):
    """75 k rows in random order: level-0 slices whose column spread exceeds 16 bits (32-bit slices in the fused down kernel),
    and chunks whose rows touch more coarse columns than the workgroup has threads (second slot loop of the kernel)"""
    from oracle.pyoracle import Oracle
    p, H = poisson_case((45, 43, 39), "left", 10)
    perms = R.level_perms(H, "random", seed=1)
    Hp = R.permute_hierarchy(H, perms)
    b = R.permute_vec(rhs(p, 1), perms[0])
    ref = Oracle(Hp.levels, sm_type="jacobi").apply(b)
    for fb in ("512", "1024"):
        dev = _dev(Hp, monkeypatch, FORCED + (("AMGX_FUSED_BLOCK", fb),))
        lp = dev.level_paths(0)
        assert lp["kernel"] == "sell" and lp["Apre_slices16"] < lp["Apre_slices"] and lp["A_slices16"] < lp["A_slices"], lp
        assert lp["max_slots"] > lp["fused_block"], lp
        assert _rel(_apply(dev, b), ref) < 1e-12
    # the same with consecutive chunks (no compact chunks): every chunk is a random set of rows
    dev = _dev(Hp, monkeypatch, (("AMGX_SELL_MAX_LANES", "1"),))
    lp = dev.level_paths(0)
    assert lp["kernel"] == "sell" and lp["compact"] == 0 and lp["max_slots"] > lp["fused_block"], lp
    assert _rel(_apply(dev, b), ref) < 1e-12


# (stencil, grid, upper diagonals K): the stencils span K = 1 .. 6; the Kuhn 3D matrix has K = 7
DIA_CASES = [("chain", (20000,), 1), ("fd5", (130, 110), 2), ("fd7", (41, 37, 29), 3), ("fd9", (130, 110), 4),
             ("offsets:1,3,64,65,500", (20000,), 5), ("offsets:1,2,7,64,130,131", (20000,), 6)]


@pytest.mark.parametrize("kind,shape,K", DIA_CASES)
def test_dia_k_matches_oracle_and_sell_path(kind, shape, K, monkeypatch):
    from oracle.pyoracle import Oracle
    A, _ = R.stencil(kind, shape, seed=K)
    H = R.hand_hierarchy(A, per_row=(2, 2), agg=8, seed=K)
    b = np.random.default_rng(K).standard_normal(A.shape[0])
    for cycle in ("V", "W"):
        dev = _dev(H, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"),), mg_cycle=cycle)
        lp = dev.level_paths(0)
        assert lp["kernel"] == "dia" and lp["dia_k"] == K and lp["ept"] == 4, lp
        x = _apply(dev, b)
        assert _rel(x, Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b)) < 1e-12
        sell = _dev(H, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_NO_DIA", "1")), mg_cycle=cycle)
        assert sell.level_paths(0)["kernel"] == "sell"
        assert _rel(x, _apply(sell, b)) < 1e-13


def test_dia_reversed_kuhn_and_refused_orderings(monkeypatch):
    """the reversed Kuhn ordering keeps its 7 upper diagonals; random and RCM orderings are refused by the detector and level 0
    keeps the SELL image with the result of AMGX_NO_DIA=1"""
    from oracle.pyoracle import Oracle
    p, H = poisson_case((41, 37, 29), "right|top", 10)
    for kind in ("reverse", "random", "rcm"):
        perms = R.level_perms(H, kind, seed=2)
        Hp = R.permute_hierarchy(H, perms)
        b = R.permute_vec(rhs(p, 1), perms[0])
        dev = _dev(Hp, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"),))
        lp = dev.level_paths(0)
        x = _apply(dev, b)
        assert _rel(x, Oracle(Hp.levels, sm_type="jacobi").apply(b)) < 1e-12
        if kind == "reverse":
            assert lp["kernel"] == "dia" and lp["dia_k"] == 7, lp
        else:
            assert lp["kernel"] != "dia" and lp["dia_k"] == 0, lp
            assert _rel(x, _apply(_dev(Hp, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"), ("AMGX_NO_DIA", "1"))), b)) < 1e-13


def test_ept6_dia(monkeypatch):
    """a prolongation with 5 entries per row: 2560 entries in a 512-row chunk, 6 per thread in the diagonal-image kernel"""
    from oracle.pyoracle import Oracle
    A, _ = R.stencil("fd7", (41, 37, 29), seed=3)
    H = R.hand_hierarchy(A, per_row=(5, 2), agg=8, seed=3)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    for env in ((), (("AMGX_COMPACT_CHUNKS_MIN_ROWS", "0"),)):
        dev = _dev(H, monkeypatch, (("AMGX_DIA_MIN_ROWS", "0"),) + env)
        lp = dev.level_paths(0)
        assert lp["kernel"] == "dia" and lp["dia_k"] == 3 and lp["ept"] == 6 and lp["compact"] == (1 if env else 0), lp
        assert _rel(_apply(dev, b), Oracle(H.levels, sm_type="jacobi").apply(b)) < 1e-12


@pytest.mark.parametrize("fb", [256, 512, 1024])
def test_ept6_sell_fused_block(fb, monkeypatch):
    from oracle.pyoracle import Oracle
    A, _ = R.stencil("fd7", (41, 37, 29), seed=4)
    H = R.hand_hierarchy(A, per_row=(5, 2), agg=8, seed=4)
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    for cycle in ("V", "W"):
        dev = _dev(H, monkeypatch, (("AMGX_SELL_MAX_LANES", "1"), ("AMGX_FUSED_BLOCK", str(fb))), mg_cycle=cycle)
        lp = dev.level_paths(0)
        assert lp["kernel"] == "sell" and lp["fused_block"] == fb and lp["lanes"] == 1 and lp["ept"] == 6, lp
        assert _rel(_apply(dev, b), Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b)) < 1e-12


def test_ept6_windowed_image(monkeypatch):
    """level 1 (the ragged aggregation level of the Kuhn problem) in the windowed form (AMGX_APRE_WINDOW=1) with a 5-entry
    prolongation below it"""
    from oracle.pyoracle import Oracle
    p, H0 = poisson_case((41, 37, 29), "right|top", 10)
    H = R.hand_hierarchy(H0.levels[0].A.to_scipy(), per_row=(5, 2), agg=8, seed=5, first_P=(H0.levels[0].P.to_scipy(),))
    b = np.random.default_rng(5).standard_normal(p.n)
    dev = _dev(H, monkeypatch, (("AMGX_SELL_MAX_LANES", "1"), ("AMGX_APRE_WINDOW", "1"), ("AMGX_NO_DENSE_TAIL", "1")))
    lp = dev.level_paths(1)
    assert lp["kernel"] == "sell-win" and lp["ept"] == 6, lp
    assert _rel(_apply(dev, b), Oracle(H.levels, sm_type="jacobi").apply(b)) < 1e-12


@pytest.mark.parametrize("G", [2, 4, 8])
def test_multi_lane_fused_restriction_with_wide_p(G, monkeypatch):
    """long rows (25 entries) in a G-lane image: with a 2-entry P the fused kernel runs with G lanes; with 4 G + 1 entries per row
    a 512 / G-row chunk holds more than 2048 entries -- amgx_create used to pick 6 entries per thread, for which no G > 1 kernel
    exists, and the first cycle threw.  Now such a level keeps the separate kernels."""
    from oracle.pyoracle import Oracle
    A, _ = R.stencil("offsets:" + ",".join(str(o) for o in range(1, 13)), (20000,), seed=G)
    env = (("AMGX_SELL_MAX_LANES", str(G)), ("AMGX_NO_LW", "1"))
    for per_row, fused in ((2, True), (4 * G + 1, False)):
        H = R.hand_hierarchy(A, per_row=(per_row, 2), agg=8, seed=G)
        b = np.random.default_rng(G).standard_normal(A.shape[0])
        for cycle in ("V", "W"):
            dev = _dev(H, monkeypatch, env, mg_cycle=cycle)
            assert dev.matrix_info(0, "Apre")["lanes"] == G
            lp = dev.level_paths(0)
            if fused:
                assert lp["kernel"] == "sell" and lp["lanes"] == G and lp["ept"] == 4 and lp["fused_block"] == 512, lp
            else:
                assert lp["kernel"] is None and lp["ept"] == 0, lp
            assert _rel(_apply(dev, b), Oracle(H.levels, sm_type="jacobi", cycle=cycle).apply(b)) < 1e-12


def test_local_window_chunks_without_window(monkeypatch):
    """a test capacity below the widest chunk: some chunks of the local-window image of A' keep global columns"""
    from oracle.pyoracle import Oracle
    p, H = poisson_case((41, 37, 29), "right|top", 10)
    for kind in ("identity", "coarse_only"):
        perms = R.level_perms(H, kind, seed=9)
        Hp = R.permute_hierarchy(H, perms)
        b = R.permute_vec(rhs(p, 1), perms[0])
        ref = Oracle(Hp.levels, sm_type="jacobi").apply(b)
        full = _dev(Hp, monkeypatch, (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1")))
        lp = full.level_paths(1)
        assert lp["kernel"] == "sell-lw" and lp["lw_no_window"] == 0, lp
        x = _apply(full, b)
        assert _rel(x, ref) < 1e-12
        for env in ((("AMGX_HOST_LW", "1"),), (("AMGX_DEV_IMAGES_MIN_ROWS", "0"),)):
            dev = _dev(Hp, monkeypatch, (("AMGX_LW_MIN_ROWS", "300"), ("AMGX_NO_DENSE_TAIL", "1"), ("AMGX_LW_TEST_CAP", "300")) + env)
            lp = dev.level_paths(1)
            assert lp["kernel"] == "sell-lw" and 0 < lp["lw_no_window"], lp
            assert _rel(_apply(dev, b), ref) < 1e-12


def _xcd_same(H, b, monkeypatch, sm_type, base_env, var, values):
    xs, paths = [], []
    for v in values:
        env = base_env + (((var, v),) if v is not None else ())
        dev = _dev(H, monkeypatch, env, sm_type=sm_type)
        xs.append(_apply(dev, b))
        paths.append(_paths(dev))
    for x in xs[1:]:
        assert np.array_equal(xs[0], x)
    return paths


@pytest.mark.parametrize("sm_type", ["jacobi", "hgs"])
def test_xcd_placement_is_bit_identical_kuhn(sm_type, monkeypatch):
    """AMGX_XCD = 0 / 2 / 3 only moves chunks between workgroups: results bit for bit equal.  Level 0 of the 2D problem has 28
    chunks (not a multiple of 8), level 1 four"""
    p, H = poisson_case((130, 110), "left|top", 5)
    b = rhs(p, 4)
    paths = _xcd_same(H, b, monkeypatch, sm_type, (("AMGX_SELL_MAX_LANES", "1"), ("AMGX_NO_DENSE_TAIL", "1")), "AMGX_XCD", ("0", "2", "3"))
    assert paths[0][0]["xcd_A"] == 0 and paths[1][0]["xcd_A"] == 1 and paths[2][0]["xcd_A"] == 1
    if sm_type == "jacobi":
        assert paths[0][0]["xcd_Apre"] == 0 and paths[1][0]["xcd_Apre"] == 1 and paths[1][0]["kernel"] == "sell"
        assert paths[1][0]["chunks"] % 8 != 0 and paths[1][1]["chunks"] < 8, paths[1][:2]


@pytest.mark.parametrize("n", [3000, 4096, 10000])
def test_xcd_placement_is_bit_identical_chunk_counts(n, monkeypatch):
    """chains with 6, 8 and 20 chunks of 512 rows: SELL with AMGX_XCD = 0 / 2 / 3, the diagonal image with AMGX_DIA_XCD"""
    A, _ = R.stencil("chain", (n,), seed=n)
    H = R.hand_hierarchy(A, per_row=(2,), agg=8, seed=1)
    b = np.random.default_rng(n).standard_normal(n)
    paths = _xcd_same(H, b, monkeypatch, "jacobi", (("AMGX_SELL_MAX_LANES", "1"),), "AMGX_XCD", ("0", "2", "3"))
    assert paths[0][0]["chunks"] == (n + 511) // 512 and paths[0][0]["kernel"] == "sell"
    assert [q[0]["xcd_Apre"] for q in paths] == [0, 1, 1]
    paths = _xcd_same(H, b, monkeypatch, "jacobi", (("AMGX_DIA_MIN_ROWS", "0"),), "AMGX_DIA_XCD", (None, "1"))
    assert paths[0][0]["kernel"] == "dia" and [q[0]["xcd_dia"] for q in paths] == [0, 1]
