"""The reference of tests/test_gpu_gs_paths.py on the CPU: the oracle's ordered hybrid Gauss-Seidel sweep (tests/hgs_oracle.py ->
oracle gs_order + gs_block) and its colour-major sweep (gs_mc) against an independent np.longdouble sweep written from the
definition, on every scalar input of the GPU file, forward and backward; and the level builders of tests/reorder.py (longest row,
symmetry, valid colourings, diagonal dominance of the block matrices)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import reorder as R

N = 6037
# relative difference oracle vs long double; the device tolerance of a Smooth is 1e-11, so this leaves a margin of 100x
SWEEP_TOL = 1e-13


def hybrid_sweep_ld(A, B, color, free, dinv, x, b, back):
    """one hybrid Gauss-Seidel sweep in long double: the free rows with a colour in the order (block of B consecutive rows, colour),
    reversed when back; x_k += dinv_k (b_k - sum_j a_kj v_j) with v_j the current value for j in the block of k and the
    sweep-start value otherwise.  It runs one colour at a time over all blocks: rows of one colour inside a block are not coupled,
    and other blocks contribute sweep-start values only, so the result is that of the row-by-row order.  B = n: one block, i.e.
    the colour-major (multicolour) sweep."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    vals = A.data.astype(np.longdouble)
    inblk = rows // B == cols // B
    col = np.where(np.asarray(free) > 0, np.asarray(color), -1)
    xo = np.asarray(x, dtype=np.longdouble)
    xn = xo.copy()
    bl = np.asarray(b, dtype=np.longdouble)
    dl = np.asarray(dinv[:n], dtype=np.longdouble)
    ent = col[rows]
    order = np.argsort(ent, kind="stable")
    sent = ent[order]
    cs = [int(c) for c in np.unique(col) if c >= 0]
    for c in (cs[::-1] if back else cs):
        lo, hi = np.searchsorted(sent, [c, c + 1])
        e = order[lo:hi]
        r = rows[e]
        v = np.where(inblk[e], xn[cols[e]], xo[cols[e]])
        starts = np.concatenate([[0], np.nonzero(np.diff(r))[0] + 1])
        s = np.add.reduceat(vals[e] * v, starts)
        k = r[starts]
        xn[k] += dl[k] * (bl[k] - s)
    return xn


def _rel(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.longdouble) - ref) / max(np.linalg.norm(ref), 1e-300))


scalar_case = R.gs_scalar_case


# every scalar input of tests/test_gpu_gs_paths.py
INPUTS = [(L, k, False, N) for L in R.GS_LENGTHS for k in R.GS_ORDERS] + \
         [(L, "identity", True, N) for L in (17, 32, 64, 128, 256)] + [(32, "identity", False, 300), (257, "identity", False, N)] + \
         [(L, "identity", False, N) for L in (3, 7, 15, 31)]


@pytest.mark.parametrize("L,kind,nonfree,n", INPUTS)
def test_builder_rows_symmetry_and_colourings(L, kind, nonfree, n):
    """the longest row has exactly L entries, A is symmetric bit for bit and diagonally dominant, the global colouring of level 0
    and the blocked colouring the device uses are valid (coupled rows differ; in-block only for the blocked one)"""
    from ngsamg_amd.device import hybrid_gs_data
    A, B, free, H = scalar_case(L, kind, nonfree, n)
    assert int(np.diff(A.indptr).max()) == L
    assert (A != A.T).nnz == 0
    d = A.diagonal()
    assert np.all(d > np.asarray(abs(A).sum(axis=1)).reshape(-1) - d)
    lv = H.levels[0]
    C = sp.coo_matrix(A)
    off = C.row != C.col
    col = np.asarray(lv.color)
    both = off & (col[C.row] >= 0) & (col[C.col] >= 0)
    assert not np.any(col[C.row][both] == col[C.col][both])
    assert np.all((col >= 0) == (free > 0)) and 0 < lv.n_colors <= 254
    if B > 0:
        hc, nc, _ = hybrid_gs_data(lv.A, free, B)
        same = both & (C.row // B == C.col // B) & (hc[C.row] >= 0) & (hc[C.col] >= 0)
        assert not np.any(hc[C.row][same] == hc[C.col][same])
        assert np.all((hc >= 0) == (free > 0)) and 0 < nc <= 254
    else:
        assert L > 256 or n <= 256


@pytest.mark.parametrize("L,kind,nonfree,n", INPUTS)
def test_oracle_sweeps_match_long_double_definition(L, kind, nonfree, n):
    """Oracle.smooth (one forward / backward sweep from a random x) against hybrid_sweep_ld: the block-hybrid order with the
    device's blocks, colours and l1-modified diagonal (gs_order + gs_block), and the colour-major order (gs_mc, plain and l1
    inverse diagonal)"""
    from ngsamg_amd.device import hybrid_gs_data
    from oracle.pyoracle import Oracle
    from tests.hgs_oracle import hgs_levels
    A, B, free, H = scalar_case(L, kind, nonfree, n)
    rng = np.random.default_rng(L)
    b = rng.standard_normal(n) * free
    x0 = rng.standard_normal(n) * free
    checks = []
    if B > 0:
        col, nc, dinv = hybrid_gs_data(H.levels[0].A, free, B)
        info = [dict(B=B, color=col, n_colors=nc, dinv=dinv), None]
        lv, types = hgs_levels(H.levels, info)
        checks.append((Oracle(lv, sm_type=types), B, col, dinv))
    checks.append((Oracle(H.levels, sm_type="gs_mc"), n, H.levels[0].color, H.levels[0].dinv))
    Hl = R.gs_hierarchy(A, free, l1_dinv=True, seed=L)
    checks.append((Oracle(Hl.levels, sm_type="gs_mc"), n, Hl.levels[0].color, Hl.levels[0].dinv))
    for orc, blk, col, dinv in checks:
        for back in (False, True):
            xo, _ = orc.smooth(0, x0.copy(), b, np.zeros(n), False, False, False, back)
            ref = hybrid_sweep_ld(A, blk, col, free, dinv, x0, b, back)
            rel = _rel(xo, ref)
            print(f"L={L} {kind} nonfree={nonfree} n={n} B={blk} back={back}: {rel:.2e}")
            assert rel <= SWEEP_TOL


@pytest.mark.parametrize("bs,L,n,odd", [(2, 151, 700, False), (3, 151, 500, False), (6, 151, 400, False), (2, 17, 700, False),
                                        (2, 25, 700, False), (2, 99, 9000, True)])
def test_block_builder(bs, L, n, odd):
    """block_long_row_matrix: symmetric bit for bit, strictly diagonally dominant by scalar rows, non-symmetric off-diagonal
    blocks, the longest block row as asked, a valid block colouring (two colours for the bipartite graph)"""
    from ngsamg_amd._lib import Matrix
    A = R.block_long_row_matrix(bs, L, n, seed=bs, odd_only=odd)
    assert (A != A.T).nnz == 0
    d = A.diagonal()
    assert np.all(d > np.asarray(abs(A).sum(axis=1)).reshape(-1) - d)
    M = Matrix.from_scipy(A, bs)
    assert int(np.diff(M.rowptr).max()) == L
    blocks = np.asarray(M.val).reshape(-1, bs, bs)
    r = np.repeat(np.arange(n), np.diff(M.rowptr))
    offd = blocks[r != M.col]
    assert np.mean([not np.allclose(E, E.T) for E in offd[:50]]) == 1.0
    color, nc = R.coloring(M)
    assert not np.any((color[r] == color[M.col]) & (r != M.col))
    if odd:
        assert nc == 2
