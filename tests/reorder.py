"""Reordered and non-Kuhn level matrices for the tests (test infrastructure; nothing in ngsamg_amd/ imports this).

permute_hierarchy(H, perms) renumbers every level of a hierarchy: A'_l = Pi_l A_l Pi_l^T, P'_l = Pi_l P_l Pi_{l+1}^T (and P^T the
same way), dinv / free / color / coords / agg by block row, columns sorted inside every row.  A permutation is given as the list
`p` of old indices in new order (new row i = old row p[i]).  Values are moved, never recomputed, so a level operator of the
result is exactly the permuted one; only summation orders of the kernels change.

permutation(kind, n, seed) makes the orderings the device formats react to, stencil(...) symmetric M-matrices on chosen
diagonals (the DIA image with K = 1 .. 7 upper diagonals), hand_hierarchy(...) a hierarchy around such a matrix with
prolongation of chosen width."""
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
