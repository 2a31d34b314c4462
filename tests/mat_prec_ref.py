"""The definition of single-precision matrix storage (mat_prec = "single"), for the tests: the level matrices the
smoother passes read are the fp64 matrices rounded to the nearest float, element by element; every vector, dinv, the transfers, the
coarse inverse and the operator of an outer Krylov iteration stay fp64.

    rounded_levels(H, levels)   copies of the hierarchy's levels with A.val passed through float32 on the listed levels
    RoundedHierarchy(H, levels) the same behind the attributes DeviceAMGMatrix and ChebyRef read from a hierarchy
    pcg(cycle, A, b)            ChebyRef.pcg with an operator of its own (the fp64 A next to a cycle on rounded levels)
"""
import copy
import dataclasses

import numpy as np

from ngsamg_amd._lib import Matrix


def rounded_levels(H, levels):
    """copies of H.levels with A.val rounded to float32 (and widened again) on the levels listed; everything else is shared"""
    src = H.levels if hasattr(H, "levels") else list(H)
    listed = {int(l) for l in levels}
    out = []
    for i, lv in enumerate(src):
        if i in listed:
            A = lv.A
            val = np.ascontiguousarray(np.asarray(A.val, dtype=np.float64).astype(np.float32).astype(np.float64))
            A = Matrix(A.n_rows, A.n_cols, A.br, A.bc, A.rowptr, A.col, val)
            if dataclasses.is_dataclass(lv):
                lv = dataclasses.replace(lv, A=A)
            else:       # (the plain namespaces of a hand-made hierarchy, tests/reorder.py)
                lv = copy.copy(lv)
                lv.A = A
        out.append(lv)
    return out


class RoundedHierarchy:
    def __init__(self, H, levels):
        self.levels = rounded_levels(H, levels)
        self.n_levels = len(self.levels)
        self.coarse_n = H.coarse_n
        self.coarse_inv = H.coarse_inv
        self.options = getattr(H, "options", None)


def smoothed_cheby_levels(H, sm="cheby"):
    """the levels a scalar mat_prec = "single" applies to: the smoothed levels whose type is "cheby" """
    n = len(H.levels)
    types = sm if isinstance(sm, (list, tuple)) else [sm] * n
    return [i for i in range(n - 1) if types[i] == "cheby"]


def pcg(cycle, A, b, tol=1e-8, maxit=200):
    """CG on the operator A (scipy matrix) with cycle.apply as preconditioner: the recurrence, the error measure
    err_k = sqrt(|<C r_k, r_k>|) and the stopping rule of ChebyRef.pcg / amgx_pcg.  Returns (x, iterations, errs)."""
    x = np.zeros_like(b, dtype=np.float64)
    d = np.array(b, dtype=np.float64)
    w = cycle.apply(d)
    s = w.copy()
    wd = float(w @ d)
    errs = [np.sqrt(abs(wd))]
    if errs[0] == 0.0:
        return x, 0, np.array(errs)
    it = 0
    for it in range(1, maxit + 1):
        q = A @ s
        alpha = wd / float(s @ q)
        x += alpha * s
        d -= alpha * q
        w = cycle.apply(d)
        wd_new = float(w @ d)
        s = w + (wd_new / wd) * s
        wd = wd_new
        errs.append(np.sqrt(abs(wd)))
        if errs[-1] <= tol * errs[0]:
            break
    return x, it, np.array(errs)
