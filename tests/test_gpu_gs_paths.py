"""Every launch-time variant of the Gauss-Seidel sweeps against the oracle's ordered sweep, on synthetic levels with chosen row
lengths (tests/reorder.py: long_row_matrix, block_long_row_matrix, gs_hierarchy).  Every case asserts through
DeviceAMGMatrix.level_paths (amgx_level_paths) that its target variant ran, and runs the operations of _operations: Smooth forward
and backward with the flag combinations of test_hgs_smoother_flag_contract, one V-cycle through Mult (the only route to the
sweep from zero, the split images and the residual + restriction kernels), and graph replay against direct launches, bitwise.

  variant                                                         test
  block-hybrid scalar (gsb_sweep_kernel<TH, G, FROM_ZERO, WP, LW>)
    G = 1 / 2 / 4 / 8 / 16 from the longest row (17 .. 256)       test_hybrid_lengths_and_orders
    general sweep: mid (WP 5) and WP 8 for G = 2 / 4 / 8 / 16     test_hybrid_lengths_and_orders (18, 33, 65, 129: mid)
    TH = 256 / 512 / 1024 for every G                             test_hybrid_threads
    from zero: narrow (WP 2) and WP 8 with the split images       test_hybrid_lengths_and_orders ("random": narrow)
      (G = 16 from zero with the split is always narrow: a block has at most 63 other rows, WP 8 needs more than 80
       in-block lower couplings per row)
    from zero over the whole image (no split, WP 8)               test_hybrid_no_split
    local-window general sweep, G = 2 / 4 / 8 / 16 (WP 8) and
      G = 4 / 8 / 16 (mid), with and without blocks that keep
      32-bit global columns                                       test_hybrid_local_window
    device-built images == host-built images, bitwise             test_hybrid_device_images_equal_host_images
    non-free rows and a whole non-free block, n % B != 0          test_hybrid_non_free_rows
    one partial block (300 rows, B = 512)                         test_hybrid_single_partial_block
    coverage of the classes above (query only)                    test_hybrid_variant_coverage
  longest row 257: multicolour form (gs_mc oracle)                test_long_rows_fall_back_to_multicolour
  multicolour scalar (gs_color_kernel<G>), G = 1 / 2 / 4 / 8 / 16,
    plain (split images) and l1 inverse diagonal (no split)       test_multicolour_scalar
  square blocks (bs = 2 / 3 / 6, 151 blocks in the longest row)
    block-hybrid and block-coloured bgsb_sweep_kernel, +- split,
      three block orderings                                       test_square_block_sweeps
    multicolour BSELL (bgs_bsell_color_kernel), +- split,
      bipartite block graph (two colours)                         test_square_block_multicolour_bsell
    multicolour row list (bgs_color_kernel<BS, W>), W = 1/2/4/8   test_square_block_multicolour_row_list
      (W = 4: a bipartite block graph, two colours of 4500 rows with 99 blocks per row)

Tolerances (the project's own): Smooth x 1e-11 max(1, |x_ref|), residual on free rows 1e-10 max(1, |r_ref|), cycles 1e-10 |ref|;
device-built vs host-built images and graph replay vs direct launches bitwise.  The reference itself is checked against a long
double sweep in tests/test_gs_paths_cpu.py."""
import numpy as np
import pytest

from tests import reorder as R

pytestmark = pytest.mark.gpu

FLAGS = ((False, False, False), (False, True, False), (True, True, True), (False, False, True))
LANE_LENGTHS = {1: 17, 2: 32, 4: 64, 8: 128, 16: 256}          # one longest row per G


def _dev(H, monkeypatch, env=(), sm_type="hgs", **kw):
    from ngsamg_amd.device import DeviceAMGMatrix
    with monkeypatch.context() as m:
        for k, v in env:
            m.setenv(k, v)
        return DeviceAMGMatrix(H, device=0, sm_type=sm_type, **kw)


def _oracle(H, dev):
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    if dev.hgs[0] is not None:
        lv, types = hgs_levels(H.levels, dev.hgs)
        return Oracle(lv, sm_type=types)
    return Oracle(H.levels, sm_type="gs_mc")


def _lanes(A):
    """Python's G: the rule of device.gs_block_rows (at most 16 entries per lane, 17 when G = 1)"""
    mx = int(np.diff(A.rowptr).max())
    return next(G for G in (1, 2, 4, 8, 16) if mx <= 16 * G + (1 if G == 1 else 0))


def _hybrid(dev, H):
    """level 0 ran the block-hybrid scalar sweep, and the device's TH is Python's B times Python's G"""
    lp = dev.level_paths(0)
    G = _lanes(H.levels[0].A)
    assert lp["gs_form"] == "hybrid", lp
    assert lp["gs_lanes"] == G and lp["gs_block"] == dev.hgs[0]["B"] and lp["gs_threads"] == dev.hgs[0]["B"] * G, lp
    return lp


def _operations(dev, H, free, seed):
    """Smooth forward / backward with every flag combination, one V-cycle (Mult) against the oracle, graph replay == direct"""
    orc = _oracle(H, dev)
    bs = H.levels[0].A.br
    A0 = H.levels[0].A.to_scipy()
    n = A0.shape[0]
    fr = np.repeat(np.asarray(free) > 0, bs)
    rng = np.random.default_rng(seed)
    for back in (False, True):
        for ru, ur, xz in FLAGS:
            b = rng.standard_normal(n) * fr
            x0 = np.zeros(n) if xz else rng.standard_normal(n) * fr
            r0 = b - A0 @ x0 if ru else rng.standard_normal(n)
            xg, rg = x0.copy(), r0.copy()
            dev.Smooth(0, xg, b, rg, ru, ur, xz, back=back)
            xo, ro = orc.smooth(0, x0.copy(), b, r0.copy(), ru, ur, xz, back)
            ex = np.linalg.norm(xg - xo) / max(1.0, np.linalg.norm(xo))
            er = np.linalg.norm((rg - ro)[fr]) / max(1.0, np.linalg.norm(ro[fr])) if ur else 0.0
            print(f"Smooth back={back} ru={ru} ur={ur} xz={xz}: x {ex:.1e} r {er:.1e}")
            assert ex <= 1e-11, (back, ru, ur, xz)
            assert er <= 1e-10, (back, ru, ur, xz)
    b = rng.standard_normal(n) * fr
    xs = []
    for graph in (True, True, False):          # capture, replay, direct launches
        x = np.full(n, np.nan)
        dev.Mult(b, x, graph=graph)
        xs.append(x)
    ref = orc.apply(b)
    ec = np.linalg.norm(xs[1] - ref) / np.linalg.norm(ref)
    print(f"cycle: {ec:.1e}")
    assert ec <= 1e-10
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[1], xs[2])


# ---- block-hybrid scalar -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", R.GS_ORDERS)
@pytest.mark.parametrize("L", R.GS_LENGTHS)
def test_hybrid_lengths_and_orders(L, kind, monkeypatch):
    """G from the longest row, default workgroups (256 lanes for G = 1, 512 otherwise), split images present; natural order:
    mostly in-block couplings, "random": mostly off-block ones (narrow sweep from zero), "slice64": in between"""
    A, B, free, H = R.gs_scalar_case(L, kind)
    dev = _dev(H, monkeypatch)
    lp = _hybrid(dev, H)
    assert lp["gs_threads"] == (256 if lp["gs_lanes"] == 1 else 512) and lp["gs_split"] == 1 and lp["gs_lw"] == 0
    print({k: v for k, v in lp.items() if k.startswith("gs_")})
    _operations(dev, H, free, L)


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_hybrid_threads(G, threads, monkeypatch):
    """AMGX_GSB_THREADS (G = 1) / AMGX_GSB_THREADS_MULTI (G > 1): TH = B G = 256, 512 or 1024 for every G"""
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], "identity")
    dev = _dev(H, monkeypatch, (("AMGX_GSB_THREADS", str(threads)), ("AMGX_GSB_THREADS_MULTI", str(threads))))
    lp = _hybrid(dev, H)
    assert lp["gs_lanes"] == G and lp["gs_threads"] == threads
    _operations(dev, H, free, threads + G)


@pytest.mark.parametrize("kind", ["identity", "random"])
@pytest.mark.parametrize("G", list(LANE_LENGTHS))
def test_hybrid_no_split(G, kind, monkeypatch):
    """AMGX_GSB_NO_SPLIT: the sweep from zero reads the whole image (WP 8, never narrow), then the full residual"""
    A, B, free, H = R.gs_scalar_case(LANE_LENGTHS[G], kind)
    dev = _dev(H, monkeypatch, (("AMGX_GSB_NO_SPLIT", "1"),))
    lp = _hybrid(dev, H)
    assert lp["gs_split"] == 0 and lp["gs_narrow"] == 0
    _operations(dev, H, free, 7 * G)


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("L", [32, 33, 64, 65, 128, 129, 256])
def test_hybrid_local_window(L, cap, monkeypatch):
    """AMGX_GSB_LW=1, AMGX_LW_MIN_ROWS=0: the general sweep reads the local-window image, G = 2 / 4 / 8 / 16 with WP 8 and
    G = 4 / 8 / 16 with the mid width (33, 65, 129; at G = 2 the mid width means at most 22 entries per row, below the 24 the
    image needs on average); cap: AMGX_LW_TEST_CAP = 3 L leaves the first and last blocks (one-sided off-block columns) a window,
    the inner blocks keep 32-bit global columns"""
    A, B, free, H = R.gs_scalar_case(L, "identity")
    env = (("AMGX_GSB_LW", "1"), ("AMGX_LW_MIN_ROWS", "0")) + ((("AMGX_LW_TEST_CAP", str(3 * L)),) if cap else ())
    dev = _dev(H, monkeypatch, env)
    lp = _hybrid(dev, H)
    G = lp["gs_lanes"]
    assert lp["gs_lw"] == 1 and lp["gs_mid"] == (L in (33, 65, 129)), lp
    nb = -(-A.shape[0] // B)
    if cap:
        assert 0 < lp["gs_lw_no_window"] < nb, lp
    else:
        assert lp["gs_lw_no_window"] == 0
    _operations(dev, H, free, 11 * G + cap)


@pytest.mark.parametrize("L", R.GS_LENGTHS)
def test_hybrid_device_images_equal_host_images(L, monkeypatch):
    """AMGX_DEV_IMAGES_MIN_ROWS=0 (+ AMGX_VERIFY_IMAGES: every device-built image against the host builder, bit for bit) against
    AMGX_HOST_IMAGES=1: the same cycle and the same sweeps bit for bit"""
    A, B, free, H = R.gs_scalar_case(L, "identity")
    dv = _dev(H, monkeypatch, (("AMGX_DEV_IMAGES_MIN_ROWS", "0"), ("AMGX_VERIFY_IMAGES", "1")))
    hs = _dev(H, monkeypatch, (("AMGX_HOST_IMAGES", "1"),))
    assert _hybrid(dv, H) == _hybrid(hs, H)
    n = A.shape[0]
    rng = np.random.default_rng(L)
    b = rng.standard_normal(n)
    xd, xh = np.full(n, np.nan), np.full(n, np.nan)
    dv.Mult(b, xd)
    hs.Mult(b, xh)
    assert np.array_equal(xd, xh)
    for back in (False, True):
        x0 = rng.standard_normal(n)
        xd, xh, rd, rh = x0.copy(), x0.copy(), np.zeros(n), np.zeros(n)
        dv.Smooth(0, xd, b, rd, False, True, False, back=back)
        hs.Smooth(0, xh, b, rh, False, True, False, back=back)
        assert np.array_equal(xd, xh) and np.array_equal(rd, rh)
    _operations(dv, H, free, L)


@pytest.mark.parametrize("L", [17, 32, 64, 128, 256])
def test_hybrid_non_free_rows(L, monkeypatch):
    """40 scattered non-free rows and one whole non-free block (their P rows empty); 6037 rows are no multiple of B"""
    A, B, free, H = R.gs_scalar_case(L, "identity", True)
    assert A.shape[0] % B != 0 and not free[3 * B:4 * B].any()
    dev = _dev(H, monkeypatch)
    _hybrid(dev, H)
    _operations(dev, H, free, L)


def test_hybrid_single_partial_block(monkeypatch):
    """300 rows, G = 2 and 1024-lane workgroups: B = 512, the level is one partial block"""
    A, B0, free, H = R.gs_scalar_case(32, "identity", False, 300)
    dev = _dev(H, monkeypatch, (("AMGX_GSB_THREADS_MULTI", "1024"),))
    lp = _hybrid(dev, H)
    assert lp["gs_block"] == 512 > A.shape[0] and lp["gs_threads"] == 1024
    _operations(dev, H, free, 300)


def test_hybrid_variant_coverage(monkeypatch):
    """the configurations of the tests above reach every (G, TH), both general-sweep widths for G > 1 (WP 8 only for G = 1), the
    narrow sweep from zero for every G and the WP 8 one with the split for G = 1 .. 8 (query only: no sweep runs here)"""
    seen = set()
    for L in R.GS_LENGTHS:
        for kind in R.GS_ORDERS:
            H = R.gs_scalar_case(L, kind)[3]
            lp = _hybrid(_dev(H, monkeypatch), H)
            seen |= {("general", lp["gs_lanes"], lp["gs_mid"]), ("zero", lp["gs_lanes"], lp["gs_narrow"]),
                     ("th", lp["gs_lanes"], lp["gs_threads"])}
    for G, L in LANE_LENGTHS.items():
        H = R.gs_scalar_case(L, "identity")[3]
        for th in (256, 512, 1024):
            lp = _hybrid(_dev(H, monkeypatch, (("AMGX_GSB_THREADS", str(th)), ("AMGX_GSB_THREADS_MULTI", str(th)))), H)
            seen.add(("th", G, lp["gs_threads"]))
    want = {("th", G, th) for G in LANE_LENGTHS for th in (256, 512, 1024)}
    want |= {("general", G, mid) for G in (2, 4, 8, 16) for mid in (0, 1)} | {("general", 1, 0)}
    want |= {("zero", G, nar) for G in (1, 2, 4, 8) for nar in (0, 1)} | {("zero", 16, 1)}
    assert want <= seen, sorted(want - seen)


def test_long_rows_fall_back_to_multicolour(monkeypatch):
    """a longest row of 257 entries: gs_block_rows gives 0, the level keeps the multicolour form (G = 16)"""
    A, B, free, H = R.gs_scalar_case(257, "identity")
    assert B == 0
    dev = _dev(H, monkeypatch)
    assert dev.hgs[0] is None
    lp = dev.level_paths(0)
    assert lp["gs_form"] == "mc" and lp["gs_lanes"] == 16 and lp["gs_split"] == 1
    _operations(dev, H, free, 257)


# ---- multicolour scalar ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("G,L", [(1, 3), (2, 7), (4, 15), (8, 31), (16, 64)])
def test_multicolour_scalar(G, L, l1, monkeypatch):
    """sm_type "gs" on a level with an average row length for G lanes (L = 3: a chain); plain inverse diagonal: the split images
    (sweep over the lower part + upper residual), l1 inverse diagonal: no split (sweep + full residual)"""
    A = R.gs_scalar_case(L, "identity")[0]
    free = np.ones(A.shape[0], np.uint8)
    H = R.gs_hierarchy(A, free, l1_dinv=l1, seed=L)
    dev = _dev(H, monkeypatch, sm_type="gs")
    lp = dev.level_paths(0)
    assert lp["gs_form"] == "mc" and lp["gs_lanes"] == G and lp["gs_split"] == (0 if l1 else 1), lp
    _operations(dev, H, free, G)


# ---- square blocks -----------------------------------------------------------------------------------------------------

BLOCK_N = {2: 700, 3: 500, 6: 400}


def _block_case(bs, L=151, n=None, odd=False, kind="identity"):
    from ngsamg_amd._lib import Matrix
    n = n or BLOCK_N[bs]
    A = R.block_long_row_matrix(bs, L, n, seed=bs + L, odd_only=odd)
    if kind != "identity":
        p = R.permutation(kind, n, seed=bs)
        A = R.permute_matrix(Matrix.from_scipy(A, bs), p, p).to_scipy()
    free = np.ones(n, np.uint8)
    free[np.random.default_rng(bs).choice(n, size=7, replace=False)] = 0
    return A, free, R.gs_hierarchy(A, free, bs=bs, seed=bs)


@pytest.mark.parametrize("kind", R.GS_ORDERS)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("coloured", [False, True])
@pytest.mark.parametrize("bs", [2, 3, 6])
def test_square_block_sweeps(bs, coloured, split, kind, monkeypatch):
    """bgsb_sweep_kernel on a level with 151 blocks in the longest row: the block-hybrid form (one launch per sweep) and the
    block-coloured one (AMGX_BGSB_BC_MIN_ROWS=0, AMGX_BGSB_BC_MIN_WG=0: one launch per block colour), with and without the split,
    in natural, random and slice64 block order"""
    A, free, H = _block_case(bs, kind=kind)
    env = (() if split else (("AMGX_BGSB_NO_SPLIT", "1"),)) + \
        ((("AMGX_BGSB_BC_MIN_ROWS", "0"), ("AMGX_BGSB_BC_MIN_WG", "0")) if coloured else ())
    dev = _dev(H, monkeypatch, env)
    lp = dev.level_paths(0)
    assert lp["gs_form"] == ("block-coloured" if coloured else "hybrid-block"), lp
    assert lp["gs_block"] == dev.hgs[0]["B"] and lp["gs_split"] == int(split)
    if coloured:
        assert lp["gs_block_colors"] == dev.hgs[0]["n_block_colors"] >= 2
    _operations(dev, H, free, bs)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("bs", [2, 3, 6])
def test_square_block_multicolour_bsell(bs, split, monkeypatch):
    """sm_type "gs" on square blocks through the colour-major BSELL copy (AMGX_BGS_BSELL_MIN=1), with and without the split
    (AMGX_NO_BGS_SPLIT); the bipartite block graph of 151 blocks per row (two colours: the copy pads every colour to whole slices,
    and the many short colours of the other levels are refused for their padding)"""
    A, free, H = _block_case(bs, odd=True)
    env = (("AMGX_BGS_BSELL_MIN", "1"),) + (() if split else (("AMGX_NO_BGS_SPLIT", "1"),))
    dev = _dev(H, monkeypatch, env, sm_type="gs")
    lp = dev.level_paths(0)
    assert lp["gs_form"] == "mc-block-bsell" and lp["gs_split"] == int(split), lp
    _operations(dev, H, free, bs)


@pytest.mark.parametrize("bs,W,L,n,odd", [(2, 1, 17, 700, False), (2, 2, 25, 700, False), (2, 4, 99, 9000, True),
                                          (2, 8, 151, 700, False), (3, 8, 151, 500, False), (6, 8, 151, 400, False)])
def test_square_block_multicolour_row_list(bs, W, L, n, odd, monkeypatch):
    """sm_type "gs" on square blocks through the CSR row list (AMGX_NO_BGS_BSELL=1): W = 1 (< 20 blocks per row), 2 (20 .. 31),
    8 (colours of at most 4096 rows, >= 32 blocks per row) and 4 (colours of more than 4096 rows, >= 48 blocks per row)"""
    A, free, H = _block_case(bs, L, n, odd)
    dev = _dev(H, monkeypatch, (("AMGX_NO_BGS_BSELL", "1"),), sm_type="gs")
    lp = dev.level_paths(0)
    assert lp["gs_form"] == "mc-block-rowlist" and lp["gs_w_mask"] == W, lp
    _operations(dev, H, free, W)
