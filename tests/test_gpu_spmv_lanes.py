"""The stand-alone SpMV family (Handle::product<1, EP>, amgx.hip): every format x lane count the host rules can pick, with the choice
asserted from the device's own report (matrix_info: fmt, lanes; level_paths: 16-bit slices, bcsr_A / bcsr_P / bcsr_PT = the
value of bcsr_kernel, the function the dispatcher calls) and the result against scipy in float64.  Synthetic matrices through
the C ABI as in test_gpu_kernel_zoo.py, whose tolerances these are: 1e-13 for products and residuals, 1e-12 for the Jacobi stages.

Sliced ELL, sell_spmv_kernel<G>, G = 1, 2, 4, 8, 16 (test_sell_lanes).  The rule doubles G while avg > 3 G and then halves it
until the padding stays below 1.35; G lanes share a row in pairs of entries, so a row of L entries is stored as
2 G ceil(ceil(L / 2) / G).  Uniform rows of 3, 6, 12, 24, 48 entries give G = 1, 2, 4, 8, 16 with two pairs per lane, one of
them half padding (rows of 5, 9, 20, 45 entries pad to 8, 16, 32, 64 and fall back to a smaller G).  Each G runs on a banded
matrix (every slice has 16-bit columns) and on one whose neighbouring rows lie at opposite ends of 130 002 columns (no slice has).

CSR-vector, csrvec_spmv_kernel<G>, G = 2 .. 64 (test_csrvec_lanes): every seventh row long; 22 x longer rows pad every sliced-ELL
candidate beyond 1.35.

Block CSR (test_square_block_rowlane, test_rectangular_rowlane, test_rectangular_csrvec, test_unit_dimension_csrvec).  Reachable
(shape, kernel, width) by the rule of bcsr_kernel -- row-per-lane iff both block dimensions are >= 2 and the block is square or
the matrix has >= 6 blocks per row; W = 1 / 2 / 4 from avg < 20 / < 48 / >= 48; else CSR-vector with G = the CSR-vector lane
count of avg within 2 .. 16:
  bcsr_rowlane_kernel   2x2, 3x3, 6x6           W = 1, 2, 4   (square level matrices whose rows are too ragged for BSELL)
                        3x6, 6x3, 2x3, 3x2      W = 1, 2, 4   (avg >= 6)
  bcsrvec_spmv_kernel   3x6, 6x3, 2x3, 3x2      G = 2, 4      (avg < 6: the lane rule gives 2 or 4 there)
                        1x2, 2x1, 1x3, 3x1, 1x6, 6x1   G = 2, 4, 8, 16
Unreachable: the CSR-vector kernel on square blocks, and its G = 8 / 16 on the rectangular shapes without a unit dimension (they
need avg > 6, where the row-per-lane kernel takes over).  All of the reachable set runs here: the transfers are P (bf x bc) and
its transpose (bc x bf) with as many coarse as fine vertices, so both have the same average and one case reaches two shapes,
through AddC2F / Prolong (P) and TransferF2C (P^T)."""
import numpy as np
import pytest
import scipy.sparse as sp

from ngsamg_amd import Matrix
from tests.test_gpu_kernel_zoo import _dev, _level, _rand_bcsr, _rel

pytestmark = pytest.mark.gpu


def _scalar_ops(dev, A, rng):
    """MatVec, JacobiPre, JacobiPost, Residual on level 0 (dinv = 1, omega = 0.9) against scipy"""
    n = A.n_rows
    S = A.to_scipy()
    for _ in range(2):
        x = rng.standard_normal(n)
        y = np.empty(n)
        dev.MatVec(0, x, y)
        assert _rel(y, S @ x) < 1e-13
    b = rng.standard_normal(n)
    x, r = np.empty(n), np.empty(n)
    dev.JacobiPre(0, b, x, r)
    assert _rel(x, 0.9 * b) < 1e-14 and _rel(r, b - S @ (0.9 * b)) < 1e-12
    xo = np.empty(n)
    dev.JacobiPost(0, x, b, xo)
    assert _rel(xo, x + 0.9 * (b - S @ x)) < 1e-12
    x = rng.standard_normal(n)
    dev.Residual(0, x, b, r)
    assert _rel(r, b - S @ x) < 1e-13


def _far_columns(rng, n, L):
    """n x n, L ascending columns in every row: near the left edge in the even rows, near the right edge in the odd ones (a random
    start within 30000 columns of the edge, random steps of 1 .. 3).  With n = 130 002 the columns of two neighbouring rows lie
    more than 65 535 apart, so no slice -- every slice holds at least four consecutive rows -- can take 16-bit column deltas."""
    off = np.cumsum(rng.integers(1, 4, size=(n, L)), axis=1) - 1
    u = rng.integers(0, 30000, size=n)
    start = np.where(np.arange(n) % 2 == 0, u, n - 3 * L - u)
    c = start[:, None] + off
    assert c.min() >= 0 and c.max() < n
    return Matrix(n, n, 1, 1, np.arange(n + 1, dtype=np.int64) * L, c.reshape(-1).astype(np.int32), rng.standard_normal(n * L))


SELL_ROW = {1: 3, 2: 6, 4: 12, 8: 24, 16: 48}


@pytest.mark.parametrize("columns", ["banded", "far"])
@pytest.mark.parametrize("lanes", list(SELL_ROW))
def test_sell_lanes(lanes, columns):
    L = SELL_ROW[lanes]
    rng = np.random.default_rng(17 * lanes + (columns == "far"))
    if columns == "banded":
        # (whole slices: the padding rows of a partial last slice lie beyond the last column, out of reach of a row-relative delta,
        #  and such a slice keeps 32-bit columns; the 130 002 rows below end in a slice of two rows or more for every G)
        A = _rand_bcsr(rng, 4992, 4992, 1, 1, lambda i: L, 2 * L)
    else:
        A = _far_columns(rng, 130002, L)       # (below 2^20 / 8 rows: the rule still doubles G up to 16)
    dev = _dev([_level(A)])
    info, lp = dev.matrix_info(0, "A"), dev.level_paths(0)
    print(info, {k: lp[k] for k in ("A_slices16", "A_slices")}, dev.matrix_info(0, "Apre"))
    assert info["fmt"] == "sell" and info["lanes"] == lanes, info
    assert lp["A_slices"] == -(-A.n_rows // (64 // lanes)), lp
    assert lp["A_slices16"] == (lp["A_slices"] if columns == "banded" else 0), lp
    _scalar_ops(dev, A, rng)


# (short rows, every seventh row, lanes): averages 2, 4, 8, 16, 32, 64 on a row count that is a multiple of 7
@pytest.mark.parametrize("short,long,lanes", [(1, 8, 2), (1, 22, 4), (2, 44, 8), (4, 88, 16), (8, 176, 32), (16, 352, 64)])
def test_csrvec_lanes(short, long, lanes):
    rng = np.random.default_rng(lanes)
    n = 7 * 428
    A = _rand_bcsr(rng, n, n, 1, 1, lambda i: short if i % 7 else long, 400)
    assert A.nnz == n * lanes
    dev = _dev([_level(A)])
    info = dev.matrix_info(0, "A")
    assert info["fmt"] == "csrvec" and info["lanes"] == lanes, info
    _scalar_ops(dev, A, rng)


# ---- block CSR -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs,avg,W", [(2, 9, 1), (2, 30, 2), (2, 60, 4), (3, 15, 1), (3, 30, 2), (3, 60, 4), (6, 8, 1), (6, 30, 2), (6, 70, 4)])
def test_square_block_rowlane(bs, avg, W):
    """ragged rows (avg / 3 .. 5 avg / 3 blocks): BSELL would pad beyond 1.30, the level matrix stays in block CSR"""
    rng = np.random.default_rng(bs * 1000 + avg)
    n = 700
    A = _rand_bcsr(rng, n, n, bs, bs, lambda i: max(1, avg + (i % 5) * (avg // 3) - (2 * avg) // 3), 150)
    lev = _level(A)
    dinv = rng.standard_normal((n, bs, bs))
    lev.dinv = np.ascontiguousarray(dinv.reshape(-1))
    dev = _dev([lev])
    info, lp = dev.matrix_info(0, "A"), dev.level_paths(0)
    assert info["fmt"] == "csrvec" and lp["bcsr_A"] == ("rowlane", W), (info, lp["bcsr_A"], A.nnz / n)
    S = A.to_scipy()
    x = rng.standard_normal(n * bs)
    y = np.empty(n * bs)
    dev.MatVec(0, x, y)
    assert _rel(y, S @ x) < 1e-13
    b = rng.standard_normal(n * bs)
    xo = np.empty(n * bs)
    dev.JacobiPost(0, x, b, xo)
    t = (b - S @ x).reshape(n, bs)
    assert _rel(xo, x + 0.9 * np.einsum("nij,nj->ni", dinv, t).reshape(-1)) < 1e-12
    r = np.empty(n * bs)
    dev.Residual(0, x, b, r)
    assert _rel(r, b - S @ x) < 1e-13


def _transfer_case(bf, bc, avg, seed):
    """two levels with as many coarse as fine vertices: P (bf x bc blocks, `avg` per row) and P^T (bc x bf, `avg` on average)"""
    rng = np.random.default_rng(seed)
    nv = 300
    P = _rand_bcsr(rng, nv, nv, bf, bc, lambda i: avg, 60)
    PTs = sp.bsr_matrix(P.to_scipy().T.tocsr(), blocksize=(bc, bf))
    PTs.sort_indices()
    PT = Matrix(nv, nv, bc, bf, PTs.indptr, PTs.indices, PTs.data)
    assert P.nnz == PT.nnz == nv * avg
    Af = _rand_bcsr(rng, nv, nv, bf, bf, lambda i: 3, 5)
    Ac = _rand_bcsr(rng, nv, nv, bc, bc, lambda i: 3, 5)
    return rng, nv, P, _dev([_level(Af, P, PT), _level(Ac)])


def _transfer_ops(dev, rng, nv, P, bf, bc):
    Ps = P.to_scipy()
    xf = rng.standard_normal(nv * bf)
    xc = np.empty(nv * bc)
    dev.TransferF2C(0, xf, xc)
    assert _rel(xc, Ps.T @ xf) < 1e-13
    xc = rng.standard_normal(nv * bc)
    a = xf.copy()
    dev.AddC2F(0, -0.3, a, xc)
    assert _rel(a, xf - 0.3 * (Ps @ xc)) < 1e-13
    out = np.empty_like(xf)
    dev.Prolong(0, 1.0, xf, xc, out)
    assert _rel(out, xf + Ps @ xc) < 1e-13


@pytest.mark.parametrize("avg,W", [(8, 1), (24, 2), (50, 4)])
@pytest.mark.parametrize("bf,bc", [(3, 6), (6, 3), (2, 3), (3, 2)])
def test_rectangular_rowlane(bf, bc, avg, W):
    rng, nv, P, dev = _transfer_case(bf, bc, avg, 100 * bf + 10 * bc + W)
    lp = dev.level_paths(0)
    assert lp["bcsr_P"] == ("rowlane", W) and lp["bcsr_PT"] == ("rowlane", W), lp
    _transfer_ops(dev, rng, nv, P, bf, bc)


@pytest.mark.parametrize("avg,G", [(5, 2), (4, 4)])
@pytest.mark.parametrize("bf,bc", [(3, 6), (6, 3), (2, 3), (3, 2)])
def test_rectangular_csrvec(bf, bc, avg, G):
    """fewer than 6 blocks per row: the lane-per-block kernel"""
    rng, nv, P, dev = _transfer_case(bf, bc, avg, 100 * bf + 10 * bc + G)
    lp = dev.level_paths(0)
    assert lp["bcsr_P"] == ("csrvec", G) and lp["bcsr_PT"] == ("csrvec", G), lp
    _transfer_ops(dev, rng, nv, P, bf, bc)


@pytest.mark.parametrize("avg", [2, 4, 8, 16])
@pytest.mark.parametrize("bf,bc", [(1, 2), (2, 1), (1, 3), (3, 1), (1, 6), (6, 1)])
def test_unit_dimension_csrvec(bf, bc, avg):
    """blocks with a unit dimension never take the row-per-lane kernel: G = avg for avg = 2, 4, 8, 16"""
    rng, nv, P, dev = _transfer_case(bf, bc, avg, 100 * bf + 10 * bc + avg)
    lp = dev.level_paths(0)
    assert lp["bcsr_P"] == ("csrvec", avg) and lp["bcsr_PT"] == ("csrvec", avg), lp
    _transfer_ops(dev, rng, nv, P, bf, bc)
