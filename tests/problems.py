"""Shared small problems for the tests (seeded, sized so the oracle finishes in seconds)."""
import functools

import numpy as np

from ngsamg_amd import fem
from ngsamg_amd._lib import Matrix
from ngsamg_amd.hierarchy import Hierarchy


def to_matrix(p):
    return Matrix(p.n, p.n, p.bs, p.bs, p.rowptr, p.col, p.val)


@functools.lru_cache(maxsize=None)
def poisson_case(shape, dirichlet="right|top", max_coarse_size=20):
    p = fem.poisson_fast(shape, dirichlet=dirichlet)
    H = Hierarchy(to_matrix(p), p.free, p.coords, dim=len(shape), energy=0, max_coarse_size=max_coarse_size)
    return p, H


@functools.lru_cache(maxsize=None)
def elasticity_case(shape, rotations=False, max_coarse_size=20, first_aaf=None):
    p = fem.elasticity_fast(shape, dirichlet="left", mu=1.0, lam=0.5, rotations=rotations)
    H = Hierarchy(to_matrix(p), p.free, p.coords, dim=len(shape), energy=1, max_coarse_size=max_coarse_size,
                  regularize_cmats=0 if rotations else 1, first_aaf=first_aaf)
    return p, H


def rhs(p, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(p.n * p.bs) * np.repeat(p.free, p.bs)


def padded_call(dev, call, arrays, device, pad=5, fill=-3.0):
    """call(k, [(address, ld), ...], flags) on column-major copies of the (k, rows) arrays with ld = rows + pad and one more
    column behind the k, as host arrays or device tensors.  Returns the (k, rows) parts after the call, having checked that
    every entry between rows and ld and in the column behind still holds `fill`."""
    k = arrays[0].shape[0]
    held = []
    for A in arrays:
        P = np.full((k + 1, A.shape[1] + pad), fill)
        P[:k, :A.shape[1]] = A
        held.append(P)
    if device:
        import torch
        held = [torch.from_numpy(P).cuda() for P in held]
        args = [(t.data_ptr(), t.shape[1]) for t in held]
    else:
        args = [(P.ctypes.data, P.shape[1]) for P in held]
    call(k, args, dev._multi_flags(device, False))
    if device:
        torch.cuda.synchronize()
        held = [t.cpu().numpy() for t in held]
    for P, A in zip(held, arrays):
        assert np.all(P[:k, A.shape[1]:] == fill) and np.all(P[k] == fill), "the call wrote outside its rows or columns"
    return [P[:k, :A.shape[1]].copy() for P, A in zip(held, arrays)]
