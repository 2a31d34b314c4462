"""Reordered and non-Kuhn level matrices for the tests (test infrastructure; nothing in ngsamg_amd/ imports this).

permute_hierarchy(H, perms) renumbers every level of a hierarchy: A'_l = Pi_l A_l Pi_l^T, P'_l = Pi_l P_l Pi_{l+1}^T (and P^T the
same way), dinv / free / color / coords / agg by block row, columns sorted inside every row.  A permutation is given as the list
`p` of old indices in new order (new row i = old row p[i]).  Values are moved, never recomputed, so a level operator of the
result is exactly the permuted one; only summation orders of the kernels change.

permutation(kind, n, seed) makes the orderings the device formats react to, stencil(...) symmetric M-matrices on chosen
diagonals (the DIA image with K = 1 .. 7 upper diagonals), hand_hierarchy(...) a hierarchy around such a matrix with
prolongation of chosen width."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from ngsamg_amd._lib import Matrix
from tests.golden_io import FixtureHierarchy

KINDS = ["identity", "reverse", "random", "slice64", "chunk512", "rcm", "coarse_only"]


def permutation(kind, n, seed=0, A=None):
    """new -> old index list of length n.  A (scipy) is needed for "rcm"."""
    rng = np.random.default_rng(seed)
    if kind in ("identity", "coarse_only"):
        return np.arange(n)
    if kind == "reverse":
        return np.arange(n)[::-1].copy()
    if kind == "random":
        return rng.permutation(n)
    if kind in ("slice64", "chunk512"):
        w = 64 if kind == "slice64" else 512
        p = np.arange(n)
        for a in range(0, n, w):
            p[a:a + w] = a + rng.permutation(min(w, n - a))
        return p
    if kind == "rcm":
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        S = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
        return np.asarray(reverse_cuthill_mckee(S, symmetric_mode=True), dtype=np.int64)
    raise ValueError(kind)


def level_perms(H, kind, seed=0):
    """one permutation per level; "coarse_only": identity on level 0, random below (scatters the columns of P_0)"""
    out = []
    for l, lv in enumerate(H.levels):
        k = "random" if kind == "coarse_only" and l > 0 else kind
        A = lv.A.to_scipy() if k == "rcm" and lv.A.br == 1 else None
        if k == "rcm" and A is None:            # block levels: RCM of the block graph
            A = sp.csr_matrix((np.ones(lv.A.nnz), lv.A.col, lv.A.rowptr), shape=(lv.A.n_rows, lv.A.n_cols))
        out.append(permutation(k, lv.A.n_rows, seed + 101 * l, A))
    return out


def inverse(p):
    q = np.empty(len(p), dtype=np.int64)
    q[np.asarray(p)] = np.arange(len(p))
    return q


def permute_matrix(M, prow, pcol):
    """M' = Pi_r M Pi_c^T in block CSR: new block row i = old block row prow[i], old block column j -> inverse(pcol)[j];
    columns sorted inside every row, blocks moved whole"""
    prow = np.asarray(prow, dtype=np.int64)
    qcol = inverse(pcol)
    rp = np.asarray(M.rowptr, dtype=np.int64)
    lens = np.diff(rp)[prow]
    new_rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # source entry of every new entry, rows in new order
    src = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in prow]) if len(prow) else np.zeros(0, dtype=np.int64)
    newcol = qcol[np.asarray(M.col)[src]]
    rowid = np.repeat(np.arange(len(prow)), lens)
    order = np.lexsort((newcol, rowid))
    src, newcol = src[order], newcol[order]
    bb = M.br * M.bc
    val = np.asarray(M.val).reshape(-1, bb)[src].reshape(-1)
    return Matrix(M.n_rows, M.n_cols, M.br, M.bc, new_rp, newcol.astype(np.int32), val)


def permute_hierarchy(H, perms):
    """the hierarchy renumbered by one permutation per level (see module docstring); a golden_io.FixtureHierarchy (dense
    coarse inverse recomputed)"""
    from ngsamg_amd.hierarchy import bgs_blocks_from_aggregates, bgs_data
    levels = []
    nl = len(H.levels)
    for l, lv in enumerate(H.levels):
        p = np.asarray(perms[l], dtype=np.int64)
        bs = lv.A.br
        A = permute_matrix(lv.A, p, p)
        P = PT = None
        agg = None
        if lv.P is not None and l + 1 < nl:
            pc = np.asarray(perms[l + 1], dtype=np.int64)
            P = permute_matrix(lv.P, p, pc)
            PT = permute_matrix(lv.PT, pc, p)
            if getattr(lv, "agg", None) is not None:
                a = np.asarray(lv.agg, dtype=np.int64)[p]
                qc = inverse(pc)
                agg = np.where(a >= 0, qc[np.maximum(a, 0)], -1).astype(np.int32)
        dinv = np.ascontiguousarray(np.asarray(lv.dinv).reshape(lv.A.n_rows, -1)[p].reshape(-1))
        color = np.ascontiguousarray(np.asarray(lv.color)[p], dtype=np.int32)
        coords = None if getattr(lv, "coords", None) is None else np.ascontiguousarray(np.asarray(lv.coords)[p])
        L = SimpleNamespace(A=A, P=P, PT=PT, free=np.ascontiguousarray(np.asarray(lv.free)[p], dtype=np.uint8), dinv=dinv,
                            color=color, n_colors=int(lv.n_colors), coords=coords, agg=agg, n=A.n_rows, bs=bs, bgs=None)
        if getattr(lv, "bgs", None) is not None and agg is not None:
            bp, br = bgs_blocks_from_aggregates(agg, L.free)
            L.bgs = bgs_data(A, bp, br, pinv=bool(getattr(getattr(H, "options", None), "regularize_cmats", 0)))
        levels.append(L)
    return FixtureHierarchy(levels)


def permute_vec(v, p, bs=1):
    return np.ascontiguousarray(np.asarray(v).reshape(-1, bs)[np.asarray(p)].reshape(-1))


# ---- stencil matrices ------------------------------------------------------------------------------------------------

def grid_offsets(kind):
    """upper neighbours (dx, dy, dz) of a finite-difference stencil on a grid in lexicographic order"""
    if kind == "chain":
        return [(1, 0, 0)]
    if kind == "fd5":
        return [(1, 0, 0), (0, 1, 0)]
    if kind == "fd7":
        return [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    if kind == "fd9":
        return [(1, 0, 0), (-1, 1, 0), (0, 1, 0), (1, 1, 0)]
    raise ValueError(kind)


def _assemble(n, I, J, w, shift):
    """symmetric M-matrix: A_ij = A_ji = -w (the same double for both), A_ii = sum_j w_ij + shift_i"""
    I, J, w = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(w, np.float64)
    rows = np.concatenate([I, J, np.arange(n)])
    cols = np.concatenate([J, I, np.arange(n)])
    deg = np.bincount(I, weights=w, minlength=n) + np.bincount(J, weights=w, minlength=n)
    vals = np.concatenate([-w, -w, deg + shift])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    return A


def stencil(kind, shape, seed=0, shift=0.05):
    """SPD M-matrix of a stencil: "chain" (1D, K = 1), "fd5" (2D 5-point, K = 2), "fd7" (3D 7-point, K = 3), "fd9" (2D
    9-point, K = 4) on a grid of `shape`, or "offsets:o1,o2,..." (1D index space of shape[0] rows, couplings i -- i + o_k).
    Random positive couplings (seeded), every mirrored pair written from one double.  Returns (scipy CSR, coords)."""
    rng = np.random.default_rng(seed)
    if kind.startswith("offsets:"):
        n = int(shape[0])
        offs = [int(v) for v in kind.split(":")[1].split(",")]
        I = np.concatenate([np.arange(n - o) for o in offs])
        J = np.concatenate([np.arange(o, n) for o in offs])
        w = rng.uniform(0.5, 1.5, size=I.size)
        coords = np.arange(n, dtype=np.float64).reshape(n, 1)
        return _assemble(n, I, J, w, shift), coords
    shape = tuple(int(s) for s in shape)
    dim = len(shape)
    n = int(np.prod(shape))
    idx = np.arange(n).reshape(shape[::-1])          # idx[z][y][x] = x + nx (y + ny z)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    coords = np.stack([grid[..., d].T.reshape(-1) for d in range(dim)], axis=1).astype(np.float64) if dim > 1 else \
        np.arange(n, dtype=np.float64).reshape(n, 1)
    I, J = [], []
    for o in grid_offsets(kind):
        o = o[:dim] if dim < 3 else o
        o = tuple(o) + (0,) * (dim - len(o))
        if dim == 1:
            src = idx[:shape[0] - o[0]] if o[0] >= 0 else idx[-o[0]:]
            dst = idx[o[0]:] if o[0] >= 0 else idx[:shape[0] + o[0]]
        else:
            # slices in (z, y, x) order of idx
            sl_s, sl_d = [], []
            for d in reversed(range(dim)):
                k = o[d]
                sl_s.append(slice(0, shape[d] - k) if k >= 0 else slice(-k, shape[d]))
                sl_d.append(slice(k, shape[d]) if k >= 0 else slice(0, shape[d] + k))
            src, dst = idx[tuple(sl_s)], idx[tuple(sl_d)]
        I.append(src.reshape(-1))
        J.append(dst.reshape(-1))
    I, J = np.concatenate(I), np.concatenate(J)
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    w = rng.uniform(0.5, 1.5, size=I.size)
    return _assemble(n, lo, hi, w, shift), coords


def upper_offsets(A):
    """the distinct upper offsets col - row > 0 of a scipy CSR matrix"""
    r = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    d = np.unique(A.indices - r)
    return [int(v) for v in d[d > 0]]


def plain_dinv(A):
    """1 / diag(A) -- the plain inverse diagonal the DIA kernel needs"""
    return np.ascontiguousarray(1.0 / A.diagonal())


def _prolongation(n, per_row, agg, rng):
    """n x ceil(n / agg): row i couples to the aggregates i // agg + k, k = 0 .. per_row - 1 (mod the coarse size), positive
    seeded weights summing to 1"""
    nc = (n + agg - 1) // agg
    cols = np.stack([(np.arange(n) // agg + k) % nc for k in range(per_row)], axis=1)
    w = rng.uniform(0.2, 1.0, size=cols.shape)
    w /= w.sum(axis=1, keepdims=True)
    P = sp.csr_matrix((w.reshape(-1), (np.repeat(np.arange(n), per_row), cols.reshape(-1))), shape=(n, nc))
    P.sum_duplicates()
    P.sort_indices()
    return P


def hand_hierarchy(A, per_row=(2,), agg=8, seed=0, first_P=()):
    """len(first_P) + len(per_row) + 1 levels around a scalar SPD matrix A (scipy CSR) without the host setup: the given
    prolongations first, then P_l with per_row[l] entries per row (_prolongation); A_{l+1} = P_l^T A_l P_l by scipy
    (symmetrised), plain inverse diagonals, every dof free, one colour (Jacobi only).  A golden_io.FixtureHierarchy."""
    rng = np.random.default_rng(seed)
    mats, Ps = [sp.csr_matrix(A)], []
    for k in list(first_P) + list(per_row):
        P = sp.csr_matrix(k) if sp.issparse(k) else _prolongation(mats[-1].shape[0], int(k), agg, rng)
        Ac = (P.T @ mats[-1] @ P).tocsr()
        Ac = ((Ac + Ac.T) * 0.5).tocsr()
        Ac.sort_indices()
        Ps.append(P)
        mats.append(Ac)
    levels = []
    for l, M in enumerate(mats):
        m = Matrix.from_scipy(M)
        P = Ps[l] if l < len(Ps) else None
        PT = None if P is None else P.T.tocsr()
        nn = m.n_rows
        levels.append(SimpleNamespace(A=m, P=None if P is None else Matrix.from_scipy(P), PT=None if PT is None else Matrix.from_scipy(PT),
                                      free=np.ones(nn, dtype=np.uint8), dinv=plain_dinv(M), color=np.zeros(nn, dtype=np.int32), n_colors=1,
                                      coords=None, agg=None, n=nn, bs=1, bgs=None))
    return FixtureHierarchy(levels)


# ---- Gauss-Seidel levels with chosen row lengths (tests/test_gpu_gs_paths.py) -------------------------------------------

GS_LENGTHS = [17, 18, 22, 23, 32, 33, 44, 45, 64, 65, 88, 89, 128, 129, 176, 177, 256]
GS_ORDERS = ["identity", "random", "slice64"]


def long_row_matrix(L, n=6037, seed=0, shift=0.05):
    """SPD M-matrix on a 1D index space whose longest row has exactly L >= 3 entries: couplings i -- i + o for o = 1 .. L // 2
    with random weights (as stencil("offsets:...")).  For even L the pairs (i, i + o) with even i and o the largest odd offset are
    dropped (every row lies in one such pair) and their weights stay on both diagonals.  Returns scipy CSR."""
    rng = np.random.default_rng(seed)
    m = L // 2
    offs = np.arange(1, m + 1)
    I = np.concatenate([np.arange(n - o) for o in offs])
    J = I + np.repeat(offs, n - offs)
    w = rng.uniform(0.5, 1.5, size=I.size)
    extra = np.zeros(n)
    if L % 2 == 0:
        o = m if m % 2 else m - 1
        drop = (J - I == o) & (I % 2 == 0)
        extra = np.bincount(I[drop], weights=w[drop], minlength=n) + np.bincount(J[drop], weights=w[drop], minlength=n)
        I, J, w = I[~drop], J[~drop], w[~drop]
    return _assemble(n, I, J, w, shift + extra)


def reorder_matrix(A, kind, seed=0):
    """Pi A Pi^T for permutation(kind) (scipy CSR, columns sorted); returns (A', p)"""
    p = permutation(kind, A.shape[0], seed, A)
    Ap = sp.csr_matrix(A)[p][:, p].tocsr()
    Ap.sort_indices()
    return Ap, p


def coloring(M, free=None):
    """a colouring of the (block) graph of M by the host library (amgh_coloring): coupled rows differ, -1 on non-free rows"""
    import ctypes as C
    from ngsamg_amd import _lib
    lib = _lib.host()
    d = M.desc()
    fr = np.ascontiguousarray(np.ones(M.n_rows, np.uint8) if free is None else free, dtype=np.uint8)
    color = np.full(M.n_rows, -1, dtype=np.int32)
    nc = C.c_int32()
    _lib.hcheck(lib.amgh_coloring(C.byref(d), _lib.ptr(fr, C.c_uint8), _lib.ptr(color, C.c_int32), C.byref(nc)))
    return color, int(nc.value)


def _block_inv_diag(A, bs, l1=False):
    """inverse of the diagonal (blocks) of a scipy matrix with bs x bs blocks; l1: of the l1-modified diagonal (adds the row sums
    of |a_ij| outside the diagonal block to its diagonal) -- not the plain inverse"""
    n = A.shape[0] // bs
    B = sp.bsr_matrix(A, blocksize=(bs, bs))
    B.sort_indices()
    r = np.repeat(np.arange(n), np.diff(B.indptr))
    D = np.zeros((n, bs, bs))
    on = B.indices == r
    D[r[on]] = B.data[on]
    if l1:
        off = np.asarray(abs(A).sum(axis=1)).reshape(n, bs) - np.abs(D).sum(axis=2)
        D = D + off[:, :, None] * np.eye(bs)[None]
    return np.ascontiguousarray(np.linalg.inv(D).reshape(-1))


def gs_hierarchy(A, free=None, bs=1, l1_dinv=False, agg=8, per_row=2, seed=0):
    """two levels around the SPD matrix A (scipy, bs x bs blocks) for the Gauss-Seidel tests: P_0 = (prolongation with per_row
    entries per row, _prolongation) x I_bs with empty rows on the non-free block rows, A_1 = P^T A P + 0.05 I (a whole non-free
    block leaves aggregates without fine rows); a valid colouring of both levels (coloring, -1 on the non-free rows); dinv the
    plain inverse diagonal (blocks), or with l1_dinv the l1-modified one on level 0.  A golden_io.FixtureHierarchy."""
    rng = np.random.default_rng(seed)
    n = A.shape[0] // bs
    free = np.ones(n, np.uint8) if free is None else np.ascontiguousarray(free, dtype=np.uint8)
    P = sp.diags(free.astype(np.float64)) @ _prolongation(n, per_row, agg, rng)
    P = sp.csr_matrix(sp.kron(P, sp.identity(bs)))
    P.eliminate_zeros()
    P.sort_indices()
    Ac = (P.T @ A @ P).tocsr()
    Ac = (((Ac + Ac.T) * 0.5) + 0.05 * sp.identity(Ac.shape[0])).tocsr()
    Ac.sort_indices()
    levels = []
    for l, (M, fr) in enumerate(((sp.csr_matrix(A), free), (Ac, np.ones(Ac.shape[0] // bs, np.uint8)))):
        m = Matrix.from_scipy(M, bs) if bs > 1 else Matrix.from_scipy(M)
        Pl = PT = None
        if l == 0:
            Pl = Matrix.from_scipy(P, bs) if bs > 1 else Matrix.from_scipy(P)
            PT = Matrix.from_scipy(P.T.tocsr(), bs) if bs > 1 else Matrix.from_scipy(P.T.tocsr())
        color, nc = coloring(m, fr)
        dinv = _block_inv_diag(M, bs, l1_dinv and l == 0) if bs > 1 else \
            (1.0 / np.asarray(abs(M).sum(axis=1)).reshape(-1) if l1_dinv and l == 0 else plain_dinv(M))
        levels.append(SimpleNamespace(A=m, P=Pl, PT=PT, free=np.ascontiguousarray(fr), dinv=np.ascontiguousarray(dinv), color=color,
                                      n_colors=nc, coords=None, agg=None, n=m.n_rows, bs=bs, bgs=None))
    return FixtureHierarchy(levels)


def nonfree_mask(n, B, seed=0, scattered=40, block=3):
    """free flags with `scattered` random non-free rows and the whole block [block * B, (block + 1) * B) non-free"""
    rng = np.random.default_rng(seed)
    free = np.ones(n, np.uint8)
    free[rng.choice(n, size=min(scattered, n), replace=False)] = 0
    free[block * B:min(n, (block + 1) * B)] = 0
    return free


def block_long_row_matrix(bs, L, n, seed=0, odd_only=False):
    """square-block SPD matrix (scipy CSR, bs x bs blocks) on the block graph of long_row_matrix(L, n) (odd_only, L odd: only the
    odd offsets 1, 3, .., L - 2 -- a bipartite graph with two colours; the longest block row still has L blocks): a random non-symmetric block E per
    edge (i, j), i < j, with A_ij = -E and A_ji = -E^T, and diagonal blocks A_ii = S_i + (row sums of |a| outside + 1) I with
    S_i random symmetric without diagonal, so that A is symmetric and strictly diagonally dominant."""
    rng = np.random.default_rng(seed)
    if odd_only:
        offs = np.arange(1, L - 1, 2)
        I = np.concatenate([np.arange(n - o) for o in offs])
        J = I + np.repeat(offs, n - offs)
    else:
        S = sp.triu(long_row_matrix(L, n, seed), k=1).tocoo()
        I, J = S.row.astype(np.int64), S.col.astype(np.int64)
    E = rng.uniform(-1.0, 1.0, size=(I.size, bs, bs))
    Sd = rng.uniform(-0.3, 0.3, size=(n, bs, bs))
    Sd = np.triu(Sd, 1)
    Sd = Sd + Sd.transpose(0, 2, 1)
    rowabs = np.zeros((n, bs))
    np.add.at(rowabs, I, np.abs(E).sum(axis=2))
    np.add.at(rowabs, J, np.abs(E).sum(axis=1))
    rowabs += np.abs(Sd).sum(axis=2)
    D = Sd + (rowabs + 1.0)[:, :, None] * np.eye(bs)[None]
    rows = np.concatenate([I, J, np.arange(n)])
    cols = np.concatenate([J, I, np.arange(n)])
    blocks = np.concatenate([-E, -E.transpose(0, 2, 1), D])
    order = np.lexsort((cols, rows))
    rows, cols, blocks = rows[order], cols[order], blocks[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    return sp.bsr_matrix((blocks, cols, indptr), shape=(n * bs, n * bs)).tocsr()


@functools.lru_cache(maxsize=None)
def gs_scalar_case(L, kind, nonfree=False, n=6037):
    """(A, B, free, hierarchy) of one scalar Gauss-Seidel input: long_row_matrix(L, n) under the ordering `kind`, B the rows per
    block gs_block_rows picks (0: multicolour), gs_hierarchy around it; nonfree: nonfree_mask (40 scattered non-free rows and
    the whole 4th block of B rows).  Cached: the tests only read it."""
    from ngsamg_amd.device import gs_block_rows
    A, _ = reorder_matrix(long_row_matrix(L, n, seed=L), kind, seed=3)
    B = gs_block_rows(Matrix.from_scipy(A))
    free = nonfree_mask(n, B or 64, seed=L) if nonfree else np.ones(n, np.uint8)
    return A, B, free, gs_hierarchy(A, free, seed=L)
