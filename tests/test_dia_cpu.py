"""Detector and host builder of the symmetric diagonal (DIA) image (amgh_dia_detect / amgh_dia_image, host/dia.hpp) --
the same code amgx_create runs to choose the level-0 image of the fused Jacobi down kernel."""
import ctypes as C

import numpy as np
import pytest

from ngsamg_amd import _lib, fem

MAX_DIAGS, MAX_FILL = 16, 1.05


def _view(n, rowptr, col, val, bs=1):
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    m = _lib.amgh_matrix(n, n, bs, bs, rowptr.ctypes.data_as(_lib.c_i64p), col.ctypes.data_as(_lib.c_i32p), val.ctypes.data_as(_lib.c_f64p))
    return m, (rowptr, col, val)


def detect(n, rowptr, col, val, bs=1):
    m, keep = _view(n, rowptr, col, val, bs)
    off = (C.c_int32 * 8)()
    K = C.c_int32()
    _lib.hcheck(_lib.host().amgh_dia_detect(C.byref(m), MAX_DIAGS, MAX_FILL, off, C.byref(K)))
    return K.value, list(off)[:max(K.value, 0)]


def image(n, rowptr, col, val, offs):
    m, keep = _view(n, rowptr, col, val)
    out = np.full(len(offs) * n, np.nan)
    o = np.asarray(offs, dtype=np.int32)
    _lib.hcheck(_lib.host().amgh_dia_image(C.byref(m), len(offs), o.ctypes.data_as(_lib.c_i32p), out.ctypes.data_as(_lib.c_f64p)))
    return out.reshape(len(offs), n)


def _rows(p):
    return np.repeat(np.arange(p.n), np.diff(p.rowptr))


SHAPES = [((41, 37, 29), "right|top"), ((45, 43, 39), "left"), ((130, 110), "left|top"), ((61, 47), "right|top"), ((70, 33), "")]


@pytest.mark.parametrize("shape,diri", SHAPES)
def test_kuhn_poisson_accepted_and_image_matches_numpy(shape, diri):
    p = fem.poisson_fast(shape, dirichlet=diri)
    K, offs = detect(p.n, p.rowptr, p.col, p.val)
    # Kuhn stencil in natural vertex order: 1 / (1, s, s + 1) in 2D, (1, s1, s1 + 1, s2, s2 + 1, s2 + s1, s2 + s1 + 1) in 3D
    d = np.unique(p.col - _rows(p))
    assert K == (7 if len(shape) == 3 else 3) and offs == [int(v) for v in d[d > 0]]
    U = image(p.n, p.rowptr, p.col, p.val, offs)
    ref = np.zeros((K, p.n))
    rows = _rows(p)
    for k, o in enumerate(offs):
        sel = p.col - rows == o
        ref[k, rows[sel]] = p.val[sel]
    assert np.array_equal(U.view(np.uint64), ref.view(np.uint64))
    # the lower couplings are the upper ones shifted: A[i][i - o] == U[k][i - o]
    for k, o in enumerate(offs):
        sel = rows - p.col == o
        assert np.array_equal(p.val[sel], U[k, p.col[sel]])


def test_one_sided_last_bit_flip_refused():
    p = fem.poisson_fast((41, 37, 29), dirichlet="right|top")
    rows = _rows(p)
    k = int(np.flatnonzero((p.col - rows == 30) & (rows > 500))[0])
    val = p.val.copy()
    val[k] = np.frombuffer((np.frombuffer(val[k].tobytes(), np.uint64) ^ np.uint64(1)).tobytes(), np.float64)[0]
    assert detect(p.n, p.rowptr, p.col, val)[0] == -5


def test_random_permutation_refused():
    import scipy.sparse as sp
    p = fem.poisson_fast((41, 37, 29), dirichlet="right|top")
    A = sp.csr_matrix((p.val, p.col, p.rowptr), shape=(p.n, p.n))
    perm = np.random.default_rng(0).permutation(p.n)
    B = A[perm][:, perm].tocsr()
    B.sort_indices()
    assert detect(p.n, B.indptr, B.indices, B.data)[0] == -2


def test_more_than_16_diagonals_refused():
    n = 500
    offs = list(range(-9, 10))                 # 19 diagonals
    rows, cols = [], []
    for i in range(n):
        for o in offs:
            if 0 <= i + o < n:
                rows.append(i)
                cols.append(i + o)
    rows, cols = np.array(rows), np.array(cols)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    val = 1.0 / (1.0 + np.abs(rows - cols))
    assert detect(n, rowptr, cols, val)[0] == -2
    # the same with 15 diagonals is accepted
    keep = np.abs(rows - cols) <= 7
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    assert detect(n, rowptr, cols[keep], val[keep]) == (7, [1, 2, 3, 4, 5, 6, 7])


def test_block_level_and_non_symmetric_pattern_refused():
    p = fem.elasticity_fast((9, 8, 7), dirichlet="left", mu=1.0, lam=0.5)
    assert detect(p.n, p.rowptr, p.col, p.val, bs=p.bs)[0] == -1
    # upper bidiagonal: offsets {0, 1} are not a symmetric set
    n = 100
    rowptr = np.concatenate([[0], np.cumsum([2] * (n - 1) + [1])])
    col = np.concatenate([[i, i + 1] for i in range(n - 1)] + [[n - 1]])
    assert detect(n, rowptr, col, np.ones(col.size))[0] == -3


# the stencil generators of tests/reorder.py: every number of upper diagonals K = 1 .. 6 the detector can give a non-Kuhn level
STENCILS = [("chain", (5000,), 1), ("fd5", (130, 110), 2), ("fd7", (41, 37, 29), 3), ("fd9", (130, 110), 4),
            ("offsets:1,3,64,65,500", (20000,), 5), ("offsets:1,2,7,64,130,131", (20000,), 6)]


@pytest.mark.parametrize("kind,shape,K", STENCILS)
def test_stencils_detected_with_their_diagonals(kind, shape, K):
    from tests import reorder as R
    A, _ = R.stencil(kind, shape, seed=K)
    offs = R.upper_offsets(A)
    assert len(offs) == K and detect(A.shape[0], A.indptr, A.indices, A.data) == (K, offs)
    if kind == "fd9":
        assert offs == [1, shape[0] - 1, shape[0], shape[0] + 1]
    U = image(A.shape[0], A.indptr, A.indices, A.data, offs)
    for k, o in enumerate(offs):
        assert np.array_equal(U[k, :A.shape[0] - o], A.diagonal(o))
    # reversal keeps the offsets (A[i][i + o] becomes A[n - 1 - i - o][n - 1 - i]: the same diagonals)
    p = R.permutation("reverse", A.shape[0])
    B = A[p][:, p].tocsr()
    B.sort_indices()
    assert detect(B.shape[0], B.indptr, B.indices, B.data) == (K, offs)
    # random orderings, and RCM orderings of the 2D / 3D grids (level sets of varying width), scatter the entries over more
    # than 16 diagonals
    for pk in ("random", "rcm") if kind.startswith("fd") else ("random",):
        p = R.permutation(pk, A.shape[0], seed=1, A=A)
        B = A[p][:, p].tocsr()
        B.sort_indices()
        assert detect(B.shape[0], B.indptr, B.indices, B.data)[0] == -2, pk


@pytest.mark.parametrize("shape", [(41, 37, 29), (130, 110)])
def test_reversed_kuhn_keeps_its_diagonals(shape):
    from tests import reorder as R
    p = fem.poisson_fast(shape, dirichlet="right|top")
    K, offs = detect(p.n, p.rowptr, p.col, p.val)
    q = R.permutation("reverse", p.n)
    from ngsamg_amd._lib import Matrix
    B = R.permute_matrix(Matrix(p.n, p.n, 1, 1, p.rowptr, p.col, p.val), q, q)
    assert detect(p.n, B.rowptr, B.col, B.val) == (K, offs) and K == (7 if len(shape) == 3 else 3)
