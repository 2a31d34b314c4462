"""amgx_mv_gram / amgx_mv_combine through the C ABI, and DeviceMultiVector against HostMultiVector.

Data are integers scaled by 1/8 ("integer-scaled"): every product is a multiple of 1/64 below 2, every sum of up to 100 003 of
them is exact in double precision.  The Gram reference is math.fsum per entry (for n > 5000: math.fsum over the sums of blocks of
1000 rows, each of which is exact); the combine reference beta * Y0 + c^T X is exact in numpy for the same reason.
Bounds (a priori, any summation order with fused multiply-add):
    Gram     |G - G_ref| <= n 2^-52 (|A|^T |B|)                        entry-wise
    combine  |Y - Y_ref| <= (kx + 2) 2^-53 (|beta| |Y0| + |X|^T |c|)    entry-wise
Row chunks of the Gram kernel are 64, 128, 256 or 512 rows (amgx_mv_gram_plan, asserted below): N has one row below / at / above
each."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from ngsamg_amd import _lib
from ngsamg_amd._lib import NgsAMGError
from ngsamg_amd.multivector import DeviceMultiVector, HostMultiVector

pytestmark = pytest.mark.gpu

N = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4097, 100003]
GRAM_K = [(1, 1), (3, 5), (8, 8), (24, 24), (32, 1), (1, 32), (32, 32)]
COMB_K = [(1, 1), (5, 3), (8, 8), (24, 8), (32, 32)]
LAYOUTS = ["cm", "cmpad", "il"]          # column-major ld = n; ld = n + 7 inside a wider, NaN-filled buffer; interleaved
PAD = 7
KMAX = 32


@pytest.fixture(scope="module")
def dev():
    from tests.problems import poisson_case
    from ngsamg_amd.device import DeviceAMGMatrix
    return DeviceAMGMatrix(poisson_case((9, 9), "left|top", 5)[1], sm_type="jacobi")


@functools.lru_cache(maxsize=None)
def _ints(n, seed):
    a = np.random.default_rng(1000 * seed + n % 997).integers(-8, 9, size=(KMAX, n)).astype(np.float64) / 8.0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _normal(n, seed):
    a = np.random.default_rng(77 * seed + n % 991).standard_normal((KMAX, n))
    a.setflags(write=False)
    return a


def _fsum_dot(a, b):
    p = a * b                                        # exact products
    if p.size <= 5000:
        return math.fsum(p)
    m = p.size // 1000 * 1000
    return math.fsum(list(p[:m].reshape(-1, 1000).sum(axis=1)) + [p[m:].sum()])     # exact block sums


@functools.lru_cache(maxsize=None)
def _gram_ref(n, sym):
    """(G_ref, |A|^T |B|) for all 32 x 32 columns of the data of size n, computed once; sym: B is A"""
    A, B = _ints(n, 1), _ints(n, 1 if sym else 2)
    G = np.array([[_fsum_dot(A[i], B[j]) for j in range(KMAX)] for i in range(KMAX)])
    return G, np.abs(A) @ np.abs(B).T


class Buf:
    """a (k, n) block placed in one of the layouts, on the host or on the device"""

    def __init__(self, block, layout, device, fill=np.nan):
        k, n = block.shape
        self.k, self.n, self.layout, self.device = k, n, layout, device
        if layout == "il":
            arr, self.ld = np.array(block.T, order="C"), 0            # (always a copy: the cached data stay as they are)
        elif layout == "cm":
            arr, self.ld = np.array(block), n
        else:                                        # rows n .. n + 6 of every column and one more column hold `fill`
            arr, self.ld = np.full((k + 1, n + PAD), fill), n + PAD
            arr[:k, :n] = block
        self.obj = torch.from_numpy(arr).cuda() if device else arr
        self.addr = self.obj.data_ptr() if device else self.obj.ctypes.data

    def host(self):
        return self.obj.cpu().numpy() if self.device else self.obj

    def block(self):
        a = self.host()
        return a.T.copy() if self.layout == "il" else a[:self.k, :self.n].copy()


def _gram(dev, A, B):
    G = np.full((A.k, B.k), np.nan)
    flags = dev._multi_flags(A.device, A.layout == "il")
    dev._ck(dev._lib.amgx_mv_gram(dev._h, A.n, A.k, A.addr, A.ld, B.k, B.addr, B.ld, _lib.ptr(G, C.c_double), flags))
    return G


def _combine(dev, X, c, beta, Y):
    c = np.ascontiguousarray(c, dtype=np.float64)
    flags = dev._multi_flags(X.device, X.layout == "il")
    dev._ck(dev._lib.amgx_mv_combine(dev._h, X.n, X.k, X.addr, X.ld, _lib.ptr(c, C.c_double), Y.k, float(beta), Y.addr, Y.ld, flags))
    if X.device:
        torch.cuda.synchronize()


def test_gram_plan_chunks_are_covered_by_the_sizes(dev):
    rc, nb = C.c_int32(), C.c_int32()
    seen = set()
    for ka, kb in GRAM_K:
        for sym in ([0, 1] if ka == kb else [0]):
            dev._ck(dev._lib.amgx_mv_gram_plan(dev._h, 100003, ka, kb, sym, C.byref(rc), C.byref(nb)))
            assert nb.value == min(1024, -(-100003 // rc.value))
            seen.add(rc.value)
    assert seen <= {64, 128, 256, 512}
    for r in seen:
        assert {r - 1, r, r + 1} <= set(N)


@pytest.mark.parametrize("ka,kb", GRAM_K)
@pytest.mark.parametrize("n", N)
def test_gram(dev, n, ka, kb):
    Gref, Gabs = _gram_ref(n, False)
    Gref, bound = Gref[:ka, :kb], n * 2.0 ** -52 * Gabs[:ka, :kb]
    a, b = _ints(n, 1)[:ka], _ints(n, 2)[:kb]
    other = Buf(_normal(200, 5)[:3], "cm", True)
    for layout in LAYOUTS:
        for device in (False, True):
            A, B = Buf(a, layout, device), Buf(b, layout, device)      # "cmpad": NaN beyond row n and beyond column k is never read
            G = _gram(dev, A, B)
            assert np.all(np.abs(G - Gref) <= bound), (layout, device, np.max(np.abs(G - Gref)))
            # the same bits when repeated, and when repeated after an unrelated call with other sizes
            An, Bn = Buf(_normal(n, 1)[:ka], layout, device), Buf(_normal(n, 2)[:kb], layout, device)
            G1 = _gram(dev, An, Bn)
            assert np.array_equal(G1, _gram(dev, An, Bn))
            _gram(dev, other, other)
            assert np.array_equal(G1, _gram(dev, An, Bn))
            # one NaN in the last row of one column: exactly its row of G
            an = np.array(a)
            ci = ka // 2
            an[ci, n - 1] = np.nan
            Gn = _gram(dev, Buf(an, layout, device), B)
            expect = np.zeros((ka, kb), dtype=bool)
            expect[ci, :] = True
            assert np.array_equal(np.isnan(Gn), expect), (layout, device)
            assert np.all(np.abs(Gn - Gref)[~expect] <= bound[~expect])
            if ka == kb:                                                 # A == B: exactly symmetric, and the general call agrees
                Sref, Sabs = _gram_ref(n, True)
                S = _gram(dev, A, A)
                assert np.array_equal(S, S.T)
                sb = n * 2.0 ** -52 * Sabs[:ka, :ka]
                assert np.all(np.abs(S - Sref[:ka, :ka]) <= sb)
                assert np.all(np.abs(_gram(dev, A, Buf(a, layout, device)) - S) <= 2 * sb)
                Sn = _gram(dev, An, An)
                assert np.array_equal(Sn, Sn.T) and np.array_equal(Sn, _gram(dev, An, An))
                sn = Buf(an, layout, device)
                Nn = _gram(dev, sn, sn)                                  # ... its row AND column
                expect = np.zeros((ka, ka), dtype=bool)
                expect[ci, :] = True
                expect[:, ci] = True
                assert np.array_equal(np.isnan(Nn), expect), (layout, device)


@pytest.mark.parametrize("kx,ky", COMB_K)
@pytest.mark.parametrize("n", N)
def test_combine(dev, n, kx, ky):
    x, y0 = _ints(n, 3)[:kx], _ints(n, 4)[:ky]
    c = np.random.default_rng(kx * 100 + ky).integers(-8, 9, size=(kx, ky)).astype(np.float64) / 8.0
    cx = c.T @ x                                     # exact (module docstring)
    cabs = np.abs(c).T @ np.abs(x)
    SENT = 7.25
    for layout in LAYOUTS:
        for device in (False, True):
            X = Buf(x, layout, device)
            for beta in (0.0, 1.0, -0.5):
                Y = Buf(y0, layout, device, fill=SENT)
                _combine(dev, X, c, beta, Y)
                bound = (kx + 2) * 2.0 ** -53 * (abs(beta) * np.abs(y0) + cabs)
                assert np.all(np.abs(Y.block() - (beta * y0 + cx)) <= bound), (layout, device, beta)
                if layout == "cmpad":               # rows >= n of the padded ld and the column beyond ky stay untouched
                    h = Y.host()
                    assert np.all(h[:ky, n:] == SENT) and np.all(h[ky] == SENT)
            Y = Buf(np.full((ky, n), np.nan), layout, device, fill=SENT)      # beta = 0 does not read Y
            _combine(dev, X, c, 0.0, Y)
            got = Y.block()
            assert np.all(np.isfinite(got)) and np.all(np.abs(got - cx) <= (kx + 2) * 2.0 ** -53 * cabs)
            if kx == ky:
                with pytest.raises(NgsAMGError, match="must not be one of the X arrays"):
                    _combine(dev, X, c, 1.0, X)


def test_argument_errors(dev):
    lib, h = dev._lib, dev._h
    a = np.zeros((33, 16))
    G = np.zeros((33, 33))
    pa, pg = a.ctypes.data, _lib.ptr(G, C.c_double)
    c = np.zeros((33, 33))
    pc = _lib.ptr(c, C.c_double)
    y = np.zeros((33, 16))
    py = y.ctypes.data

    def err():
        return lib.amgx_last_error(h).decode()
    for ka, kb in ((0, 1), (1, 0), (33, 1), (1, 33), (-1, 1)):
        assert lib.amgx_mv_gram(h, 16, ka, pa, 16, kb, pa, 16, pg, 0) != 0 and "AMGX_MV_MAX" in err()
        assert lib.amgx_mv_combine(h, 16, ka, pa, 16, pc, kb, 0.0, py, 16, 0) != 0 and "AMGX_MV_MAX" in err()
    assert lib.amgx_mv_gram(h, 16, 2, pa, 15, 2, pa, 16, pg, 0) != 0 and "leading dimension" in err()
    assert lib.amgx_mv_gram(h, 16, 2, pa, 16, 2, pa, 15, pg, 0) != 0 and "leading dimension" in err()
    assert lib.amgx_mv_gram(h, 16, 2, pa, 0, 2, pa, 0, pg, _lib.AMGX_MULTI_INTERLEAVED) == 0          # ld is ignored
    assert lib.amgx_mv_combine(h, 16, 2, pa, 15, pc, 2, 0.0, py, 16, 0) != 0 and "leading dimension" in err()
    assert lib.amgx_mv_combine(h, 16, 2, pa, 16, pc, 2, 0.0, py, 15, 0) != 0 and "leading dimension" in err()
    assert lib.amgx_mv_gram(h, 16, 2, None, 16, 2, pa, 16, pg, 0) != 0 and "null" in err()
    assert lib.amgx_mv_gram(h, 16, 2, pa, 16, 2, None, 16, pg, 0) != 0 and "null" in err()
    assert lib.amgx_mv_gram(h, 16, 2, pa, 16, 2, pa, 16, None, 0) != 0 and "null" in err()
    assert lib.amgx_mv_combine(h, 16, 2, None, 16, pc, 2, 0.0, py, 16, 0) != 0 and "null" in err()
    assert lib.amgx_mv_combine(h, 16, 2, pa, 16, None, 2, 0.0, py, 16, 0) != 0 and "null" in err()
    assert lib.amgx_mv_combine(h, 16, 2, pa, 16, pc, 2, 0.0, None, 16, 0) != 0 and "null" in err()
    assert lib.amgx_mv_gram(h, -1, 2, pa, 16, 2, pa, 16, pg, 0) != 0 and "negative" in err()
    assert lib.amgx_mv_combine(h, -1, 2, pa, 16, pc, 2, 0.0, py, 16, 0) != 0 and "negative" in err()
    assert lib.amgx_mv_gram(None, 16, 2, pa, 16, 2, pa, 16, pg, 0) != 0
    # n = 0: a zero G, combine returns at once (null vectors are fine)
    G[:] = 5.0
    assert lib.amgx_mv_gram(h, 0, 2, None, 0, 3, None, 0, pg, 0) == 0
    assert not G.reshape(-1)[:6].any() and np.all(G.reshape(-1)[6:] == 5.0)
    assert lib.amgx_mv_combine(h, 0, 2, None, 0, pc, 2, 1.0, None, 0, 0) == 0


def _pair(dev, block):
    return HostMultiVector(np.array(block)), DeviceMultiVector(dev, torch.from_numpy(np.array(block)).cuda())


def test_device_multivector_matches_host(dev):
    n = 4097
    a, b = _ints(n, 1)[:6], _ints(n, 2)[:11]
    Ha, Da = _pair(dev, a)
    Hb, Db = _pair(dev, b)
    assert (Da.k, Da.n, Da.ld) == (6, n, n)
    G = Da.InnerProduct(Db)
    assert np.all(np.abs(G - Ha.InnerProduct(Hb)) <= n * 2.0 ** -52 * (np.abs(a) @ np.abs(b).T))
    S = Da.InnerProduct(Da)
    assert np.array_equal(S, S.T)
    V = Db[2:7]                                        # a view: no copy, columns 2 .. 6
    assert V.data.data_ptr() == Db.data[2].data_ptr() and V.k == 5
    assert np.array_equal(Da.InnerProduct(V), G[:, 2:7])
    c = np.random.default_rng(3).integers(-8, 9, size=(6, 4)).astype(np.float64) / 8.0
    for beta in (0.0, 1.0, -0.5):
        Hy, Dy = _pair(dev, _ints(n, 4)[:4])
        y0 = Hy.data.copy()
        Ha.Combine(c, out=Hy, beta=beta)
        Da.Combine(c, out=Dy, beta=beta)
        bound = 8 * 2.0 ** -53 * (abs(beta) * np.abs(y0) + np.abs(c).T @ np.abs(a))
        assert np.all(np.abs(Dy.data.cpu().numpy() - Hy.data) <= bound)
    assert np.array_equal((Da * c).data.cpu().numpy(), Da.Combine(c).data.cpu().numpy())
    with pytest.raises(NgsAMGError, match="must not be"):
        Da.Combine(np.eye(6), out=Da)
    with pytest.raises(NgsAMGError, match="must not be"):
        Da.Combine(np.ones((6, 2)), out=Da[1:3])
    Da[0:2].Combine(np.eye(2), out=Da[2:4])
    got = Da.data.cpu().numpy()
    assert np.array_equal(got[2:4], got[0:2])
    # Scale / Mask / Gather / Scatter / Copy follow the host class
    free = (np.arange(n) % 5 != 0).astype(np.float64)
    for H_, D_ in (_pair(dev, _normal(n, 6)[:3]),):
        H_.Scale([2.0, -1.0, 0.5]).Mask(free)
        D_.Scale([2.0, -1.0, 0.5]).Mask(free)
        assert np.array_equal(D_.data.cpu().numpy(), H_.data)
        assert np.array_equal(D_.Gather([2, 0]).data.cpu().numpy(), H_.Gather([2, 0]).data)
        assert np.array_equal(D_.Copy().data.cpu().numpy(), H_.data)
        assert np.array_equal(D_.randn_like(2, 5).data.cpu().numpy(), H_.randn_like(2, 5).data)
    wide = DeviceMultiVector(dev, torch.zeros((33, 8), dtype=torch.float64, device="cuda"))
    with pytest.raises(NgsAMGError, match="AMGX_MV_MAX"):
        wide.InnerProduct(wide.zeros_like(1))


def test_device_orthonormalize(dev):
    from tests.test_multivector_cpu import _conditioned_block
    a = _conditioned_block(6, 4097, 1e6, 7)
    D = DeviceMultiVector(dev, torch.from_numpy(a).cuda())
    assert D.Orthonormalize() is True
    x = D.data.cpu().numpy()
    assert np.max(np.abs(x @ x.T - np.eye(6))) <= 1e-13
    b = np.array(_normal(300, 2)[:4])
    b[3] = b[1]
    D = DeviceMultiVector(dev, torch.from_numpy(b).cuda())
    assert D.Orthonormalize() is False
    assert np.array_equal(D.data.cpu().numpy(), b)
