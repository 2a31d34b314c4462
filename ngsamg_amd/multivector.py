"""Multi-vectors with NGSolve's MultiVector surface, in two interchangeable backends.

    HostMultiVector(array (k, n))            numpy only
    DeviceMultiVector(dev, tensor (k, n))    a torch CUDA tensor and a DeviceAMGMatrix, whose handle serves the two device
                                             primitives amgx_mv_gram (InnerProduct) and amgx_mv_combine (Combine)

Row j of the (k, n) array is vector j (column-major multi-vector with ld = the row stride).  Everything a block eigensolver
needs (ngsamg_amd.eigen) is written over this surface once: InnerProduct, Combine, slicing views, Copy / Scale / Mask,
Orthonormalize.  MultMulti / MatVecMulti are the matching operator adapters (apply_block(mv_in, mv_out)).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NgsAMGError

EPS = 2.0 ** -52


class _MultiVectorBase:
    """What both backends share: everything that is a composition of InnerProduct, Combine and copies."""

    def __len__(self):
        return self.k

    def __mul__(self, c):
        return self.Combine(c)

    def _coeff(self, c, name="c"):
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float64))
        if c.ndim == 1:
            c = c.reshape(-1, 1)
        if c.ndim != 2 or c.shape[0] != self.k or c.shape[1] < 1:
            raise NgsAMGError(f"{name}: need a ({self.k}, k') matrix, got shape {c.shape}")
        return c

    def _slice(self, key):
        if not isinstance(key, slice):
            raise NgsAMGError("multi-vector views are taken with a slice of the columns")
        a, b, step = key.indices(self.k)
        if step != 1 or b <= a:
            raise NgsAMGError("multi-vector views need a non-empty slice with step 1")
        return a, b

    def Orthonormalize(self, ipvec=None, carry=()):
        """Orthonormalise the columns in the inner product <x, y> = x . (M y), ipvec = M * self (None: M = I): Cholesky of the
        (diagonally scaled) Gram matrix on the host, Combine with the inverse factor, applied twice (CholQR2).  ipvec and every
        multi-vector in `carry` (A * self, ...) are transformed alike.  Returns False -- it does not raise -- when the Gram
        matrix is not positive definite to working precision; the multi-vectors are then as the last complete pass left them
        (untouched when the first pass fails)."""
        from scipy.linalg import cholesky, solve_triangular, LinAlgError
        k = self.k
        group = [self] + ([ipvec] if ipvec is not None else []) + list(carry)
        for _ in range(2):
            G = self.InnerProduct(self if ipvec is None else ipvec)
            d = np.diag(G).copy()
            if not np.all(np.isfinite(G)) or np.any(d <= 0.0):
                return False
            s = 1.0 / np.sqrt(d)
            Gs = 0.5 * (G + G.T) * np.outer(s, s)
            try:
                L = cholesky(Gs, lower=True)
            except (LinAlgError, ValueError):
                return False
            if not np.all(np.isfinite(L)) or np.min(np.diag(L)) ** 2 <= k * EPS:
                return False
            c = s[:, None] * solve_triangular(L, np.eye(k), lower=True).T      # D^-1/2 L^-T
            for v in group:
                v.Assign(v.Combine(c))
        return True


class HostMultiVector(_MultiVectorBase):
    def __init__(self, array):
        a = np.asarray(array)
        if a.ndim != 2 or a.dtype != np.float64 or a.shape[0] < 1:
            raise NgsAMGError("HostMultiVector: need a 2-D float64 array of shape (k, n)")
        if a.shape[1] > 1 and a.strides[1] != 8:
            raise NgsAMGError("HostMultiVector: the vectors (rows) must be contiguous")
        self.data = a

    k = property(lambda self: self.data.shape[0])
    n = property(lambda self: self.data.shape[1])

    def __getitem__(self, key):
        a, b = self._slice(key)
        return HostMultiVector(self.data[a:b])

    def zeros_like(self, k):
        return HostMultiVector(np.zeros((int(k), self.n)))

    def randn_like(self, k, seed=0):
        return HostMultiVector(np.random.default_rng(seed).standard_normal((int(k), self.n)))

    def Copy(self):
        return HostMultiVector(self.data.copy())

    def Assign(self, other):
        self.data[...] = other.data
        return self

    def Gather(self, cols):
        return HostMultiVector(self.data[np.asarray(cols, dtype=np.int64)].copy())

    def Scatter(self, cols, src):
        self.data[np.asarray(cols, dtype=np.int64)] = src.data
        return self

    def Scale(self, vec):
        self.data *= np.asarray(vec, dtype=np.float64).reshape(self.k, 1)
        return self

    def Mask(self, free):
        if free is not None:
            self.data *= np.asarray(free, dtype=np.float64).reshape(1, self.n)
        return self

    def InnerProduct(self, other):
        if other.n != self.n:
            raise NgsAMGError("InnerProduct: the multi-vectors have different lengths")
        G = self.data @ other.data.T
        return 0.5 * (G + G.T) if other is self else G

    def Combine(self, c, out=None, beta=0.0):
        c = self._coeff(c)
        if out is None:
            out, beta = self.zeros_like(c.shape[1]), 0.0
        if out.k != c.shape[1] or out.n != self.n:
            raise NgsAMGError("Combine: out has the wrong shape")
        if np.shares_memory(out.data, self.data):
            raise NgsAMGError("Combine: out must not be (a view of) the multi-vector that is combined")
        if beta == 0.0:
            out.data[...] = c.T @ self.data
        else:
            out.data *= beta
            out.data += c.T @ self.data
        return out


class DeviceMultiVector(_MultiVectorBase):
    def __init__(self, dev, tensor):
        import torch
        t = tensor
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[0] >= 1):
            raise NgsAMGError("DeviceMultiVector: need a 2-D float64 CUDA tensor of shape (k, n)")
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise NgsAMGError("DeviceMultiVector: the vectors (rows) must be contiguous")
        if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
            raise NgsAMGError("DeviceMultiVector: overlapping rows")
        self.dev = dev
        self.data = t

    k = property(lambda self: int(self.data.shape[0]))
    n = property(lambda self: int(self.data.shape[1]))

    @property
    def ld(self):
        return int(self.data.stride(0)) if self.k > 1 else max(self.n, 1)

    def _span(self):
        a = self.data.data_ptr()
        return a, a + 8 * ((self.k - 1) * self.ld + self.n)

    def _flags(self):
        return self.dev._multi_flags(True, False)

    def _check_k(self, k, what):
        if not (1 <= k <= _lib.AMGX_MV_MAX):
            raise NgsAMGError(f"{what}: {k} columns, need 1 .. AMGX_MV_MAX = {_lib.AMGX_MV_MAX}")

    def __getitem__(self, key):
        a, b = self._slice(key)
        return DeviceMultiVector(self.dev, self.data[a:b])

    def zeros_like(self, k):
        import torch
        return DeviceMultiVector(self.dev, torch.zeros((int(k), self.n), dtype=torch.float64, device=self.data.device))

    def randn_like(self, k, seed=0):
        import torch
        host = np.random.default_rng(seed).standard_normal((int(k), self.n))      # the numbers of HostMultiVector.randn_like
        return DeviceMultiVector(self.dev, torch.from_numpy(host).to(self.data.device))

    def Copy(self):
        return DeviceMultiVector(self.dev, self.data.clone().contiguous())

    def Assign(self, other):
        self.data.copy_(other.data)
        return self

    def Gather(self, cols):
        import torch
        idx = torch.as_tensor(np.asarray(cols, dtype=np.int64), device=self.data.device)
        return DeviceMultiVector(self.dev, self.data.index_select(0, idx).contiguous())

    def Scatter(self, cols, src):
        import torch
        idx = torch.as_tensor(np.asarray(cols, dtype=np.int64), device=self.data.device)
        self.data.index_copy_(0, idx, src.data)
        return self

    def Scale(self, vec):
        import torch
        v = torch.as_tensor(np.asarray(vec, dtype=np.float64).reshape(self.k, 1), device=self.data.device)
        self.data.mul_(v)
        return self

    def Mask(self, free):
        if free is not None:
            import torch
            if not hasattr(free, "is_cuda"):
                free = torch.as_tensor(np.asarray(free, dtype=np.float64), device=self.data.device)
            self.data.mul_(free.reshape(1, self.n))
        return self

    def InnerProduct(self, other):
        if other.n != self.n:
            raise NgsAMGError("InnerProduct: the multi-vectors have different lengths")
        self._check_k(self.k, "InnerProduct")
        self._check_k(other.k, "InnerProduct")
        G = np.empty((self.k, other.k))
        d = self.dev
        d._ck(d._lib.amgx_mv_gram(d._h, self.n, self.k, self.data.data_ptr(), self.ld, other.k, other.data.data_ptr(), other.ld,
                                  _lib.ptr(G, C.c_double), self._flags()))
        return G

    def Combine(self, c, out=None, beta=0.0):
        c = self._coeff(c)
        if out is None:
            out, beta = self.zeros_like(c.shape[1]), 0.0
        if out.k != c.shape[1] or out.n != self.n:
            raise NgsAMGError("Combine: out has the wrong shape")
        self._check_k(self.k, "Combine")
        self._check_k(out.k, "Combine")
        (a0, a1), (b0, b1) = self._span(), out._span()
        if a0 < b1 and b0 < a1:
            raise NgsAMGError("Combine: out must not be (a view of) the multi-vector that is combined")
        d = self.dev
        d._ck(d._lib.amgx_mv_combine(d._h, self.n, self.k, self.data.data_ptr(), self.ld, _lib.ptr(c, C.c_double), out.k, float(beta),
                                     out.data.data_ptr(), out.ld, self._flags()))
        return out


# ---------------------------------------------------------------------------------------------------
# operator adapters: apply_block(mv_in, mv_out) on either backend
# ---------------------------------------------------------------------------------------------------

class _BlockOp:
    """Runs an operator of a DeviceAMGMatrix on the columns of a multi-vector, at most 8 (AMGX_MULTI_MAX) per call.  An object
    that has apply_block(mv_in, mv_out) itself is passed through.  `columns` counts the columns seen."""

    def __init__(self, op, fuse=False):
        from .device import check_fuse
        check_fuse(fuse)
        self.op = op
        self.fuse = fuse if isinstance(fuse, str) else bool(fuse)
        self.columns = 0
        self.calls = 0

    def _call(self, X, Y, fuse):
        raise NotImplementedError

    def apply_block(self, mv_in, mv_out, fuse=None):
        if mv_in.k != mv_out.k:
            raise NgsAMGError("apply_block: the multi-vectors have different numbers of columns")
        self.columns += mv_in.k
        self.calls += 1
        if hasattr(self.op, "apply_block"):
            self.op.apply_block(mv_in, mv_out)
            return mv_out
        fuse = self.fuse if fuse is None else (fuse if isinstance(fuse, str) else bool(fuse))
        step = _lib.AMGX_MULTI_MAX
        for a in range(0, mv_in.k, step):
            b = min(a + step, mv_in.k)
            X, Y = mv_in.data[a:b], mv_out.data[a:b]
            if not (_contiguous(X) and _contiguous(Y)):
                raise NgsAMGError("apply_block: need multi-vectors whose columns lie back to back (ld = n)")
            self._call(X, Y, fuse)
        return mv_out

    def zeros(self, k):
        """a device multi-vector of k zero columns of the operator's size"""
        import torch
        dev = self.op
        t = torch.zeros((int(k), dev.sizes[0]), dtype=torch.float64, device=f"cuda:{dev._cfg.get('device', 0)}")
        return DeviceMultiVector(dev, t)


def _contiguous(a):
    return a.is_contiguous() if hasattr(a, "is_contiguous") else bool(a.flags.c_contiguous)


class MultMulti(_BlockOp):
    """mv_out = C mv_in, the cycle of a DeviceAMGMatrix (amgx_apply_multi)"""

    def _call(self, X, Y, fuse):
        self.op.MultMulti(X, Y, fuse=fuse)


class MatVecMulti(_BlockOp):
    """mv_out = A_level mv_in (amgx_matvec_multi)"""

    def __init__(self, level, op, fuse=False):
        super().__init__(op, fuse)
        self.level = int(level)

    def _call(self, X, Y, fuse):
        self.op.MatVecMulti(self.level, X, Y, fuse=fuse)
