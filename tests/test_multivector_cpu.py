"""HostMultiVector (ngsamg_amd.multivector) against plain numpy, and the operator adapters' column chunking."""
import numpy as np
import pytest

from ngsamg_amd._lib import NgsAMGError
from ngsamg_amd.multivector import HostMultiVector, MatVecMulti, MultMulti


def _mv(k, n, seed=0):
    return HostMultiVector(np.random.default_rng(seed).standard_normal((k, n)))


def test_sizes_and_views():
    X = _mv(5, 37)
    assert (X.k, X.n, len(X)) == (5, 37, 5)
    V = X[1:4]
    assert (V.k, V.n) == (3, 37)
    V.data[0, 0] = 123.0                                # a view, not a copy
    assert X.data[1, 0] == 123.0
    assert np.shares_memory(V.data, X.data)
    assert not np.shares_memory(X.Copy().data, X.data)
    for bad in (slice(0, 5, 2), slice(3, 3), 2):
        with pytest.raises(NgsAMGError):
            X[bad]
    Z = X.zeros_like(3)
    assert Z.data.shape == (3, 37) and not Z.data.any()
    assert np.array_equal(X.randn_like(2, 11).data, X.randn_like(2, 11).data)


def test_inner_product_matches_numpy():
    X, Y = _mv(4, 101, 1), _mv(7, 101, 2)
    G = X.InnerProduct(Y)
    assert G.shape == (4, 7)
    assert np.allclose(G, X.data @ Y.data.T, rtol=0, atol=1e-13)
    S = X.InnerProduct(X)
    assert np.array_equal(S, S.T)
    with pytest.raises(NgsAMGError):
        X.InnerProduct(_mv(4, 100))


@pytest.mark.parametrize("beta", [0.0, 1.0, -0.5])
def test_combine_matches_numpy(beta):
    X = _mv(5, 83, 3)
    c = np.random.default_rng(4).standard_normal((5, 3))
    Y = _mv(3, 83, 5)
    y0 = Y.data.copy()
    out = X.Combine(c, out=Y, beta=beta)
    assert out is Y
    assert np.allclose(Y.data, beta * y0 + c.T @ X.data, rtol=0, atol=1e-13)
    assert np.allclose((X * c).data, c.T @ X.data, rtol=0, atol=1e-13)


def test_combine_beta_zero_does_not_read_out():
    X = _mv(2, 20)
    Y = HostMultiVector(np.full((2, 20), np.nan))
    X.Combine(np.eye(2), out=Y, beta=0.0)
    assert np.array_equal(Y.data, X.data)


def test_combine_refuses_aliasing_and_bad_shapes():
    X = _mv(4, 30)
    with pytest.raises(NgsAMGError, match="must not be"):
        X.Combine(np.eye(4), out=X)
    with pytest.raises(NgsAMGError, match="must not be"):
        X.Combine(np.ones((4, 2)), out=X[1:3])
    X[0:2].Combine(np.eye(2), out=X[2:4])               # disjoint views of one array are fine
    assert np.array_equal(X.data[2:4], X.data[0:2])
    with pytest.raises(NgsAMGError):
        X.Combine(np.ones((3, 2)))
    with pytest.raises(NgsAMGError):
        X.Combine(np.ones((4, 2)), out=_mv(3, 30))


def test_scale_mask_gather_scatter():
    X = _mv(3, 17)
    x0 = X.data.copy()
    X.Scale([2.0, -1.0, 0.5])
    assert np.array_equal(X.data, x0 * np.array([[2.0], [-1.0], [0.5]]))
    free = (np.arange(17) % 3 != 0).astype(np.uint8)
    x1 = X.data.copy()
    X.Mask(free)
    assert np.array_equal(X.data, x1 * free)
    assert X.Mask(None) is X
    G = X.Gather([2, 0])
    assert np.array_equal(G.data, X.data[[2, 0]])
    X.Scatter([1], HostMultiVector(np.ones((1, 17))))
    assert np.array_equal(X.data[1], np.ones(17))


def _conditioned_block(k, n, cond, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    V, _ = np.linalg.qr(rng.standard_normal((k, k)))
    s = np.logspace(0, -np.log10(cond), k)
    return np.ascontiguousarray(((Q * s) @ V.T).T)


def test_orthonormalize_ill_conditioned_block():
    a = _conditioned_block(6, 400, 1e6, 7)
    assert 5e5 < np.linalg.cond(a) < 2e6
    X = HostMultiVector(a.copy())
    assert X.Orthonormalize() is True
    G = X.data @ X.data.T
    assert np.max(np.abs(G - np.eye(6))) <= 1e-13
    # the span is kept
    assert np.linalg.matrix_rank(np.vstack([a, X.data]), tol=1e-9) == 6


def test_orthonormalize_with_inner_product_and_carry():
    rng = np.random.default_rng(8)
    n = 120
    m = rng.uniform(0.5, 2.0, n)
    a = rng.standard_normal((4, n))
    X, MX, AX = HostMultiVector(a.copy()), HostMultiVector(a * m), HostMultiVector(3.0 * a)
    assert X.Orthonormalize(MX, carry=[AX])
    assert np.max(np.abs(X.data @ (m * X.data).T - np.eye(4))) <= 1e-13
    assert np.allclose(MX.data, m * X.data, rtol=0, atol=1e-12)
    assert np.allclose(AX.data, 3.0 * X.data, rtol=0, atol=1e-12)


def test_orthonormalize_rank_deficient_block_returns_false():
    a = np.random.default_rng(9).standard_normal((4, 50))
    a[3] = a[1]                                          # exactly rank deficient
    X = HostMultiVector(a.copy())
    assert X.Orthonormalize() is False
    assert np.array_equal(X.data, a)                     # the first pass failed: untouched
    b = np.random.default_rng(10).standard_normal((3, 50))
    b[2] = 2.0 * b[0] - 3.0 * b[1]
    assert HostMultiVector(b).Orthonormalize() is False
    z = np.random.default_rng(11).standard_normal((3, 50))
    z[1] = 0.0
    assert HostMultiVector(z).Orthonormalize() is False


class _Recorder:
    """stands in for a DeviceAMGMatrix: records the shapes of the calls"""

    def __init__(self):
        self.calls = []

    def MultMulti(self, B, X, fuse=False):
        self.calls.append(("mult", B.shape[0], fuse))
        X[...] = 2.0 * B

    def MatVecMulti(self, level, X, Y, fuse=False):
        self.calls.append(("matvec", level, X.shape[0], fuse))
        Y[...] = 3.0 * X


def test_adapters_cut_wide_blocks_and_pass_fuse():
    X, Y = _mv(19, 12), _mv(19, 12, 1)
    r = _Recorder()
    op = MultMulti(r, fuse=True)
    op.apply_block(X, Y)
    assert r.calls == [("mult", 8, True), ("mult", 8, True), ("mult", 3, True)]
    assert np.array_equal(Y.data, 2.0 * X.data)
    assert (op.columns, op.calls) == (19, 1)
    r.calls.clear()
    mv = MatVecMulti(0, r)
    mv.apply_block(X[0:5], Y[0:5])
    mv.apply_block(X[0:5], Y[0:5], fuse=True)
    assert r.calls == [("matvec", 0, 5, False), ("matvec", 0, 5, True)]
    assert np.array_equal(Y.data[0:5], 3.0 * X.data[0:5])
    with pytest.raises(NgsAMGError):
        MultMulti(r, fuse=1)
    with pytest.raises(NgsAMGError):
        op.apply_block(X[0:2], Y[0:3])

    class Own:
        def apply_block(self, a, b):
            b.data[...] = -a.data
    MultMulti(Own()).apply_block(X, Y)                   # an object with apply_block is passed through
    assert np.array_equal(Y.data, -X.data)
