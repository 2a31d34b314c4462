"""Block eigensolver (LOBPCG / PINVIT) over the multi-vector surface of ngsamg_amd.multivector.

The loop is the one of ngsolve.eigenvalues (PINVIT / LOBPCG: a Python loop over MultiVector.InnerProduct, MultiVector * matrix
and Orthogonalize); it runs unchanged on HostMultiVector (numpy) and DeviceMultiVector (amgx_mv_gram, amgx_mv_combine,
amgx_matvec_multi, amgx_apply_multi).  Only the small Rayleigh-Ritz problems are solved on the host (scipy.linalg.eigh).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import NgsAMGError
from .multivector import EPS, _BlockOp

REFRESH = 20          # iterations between two recomputations of A X (and M X) from X: the carried products drift


def _apply(op, X, Y, fuse):
    if isinstance(op, _BlockOp):
        return op.apply_block(X, Y, fuse=fuse)
    return op.apply_block(X, Y)


def _ritz(GA, GM, m):
    """smallest eigenpairs of the pencil (GA, GM), both symmetrised; None when the basis is rank deficient to working precision
    (smallest eigenvalue of GM below m 2^-52 |GM|) or the solver raises"""
    from scipy.linalg import eigh, LinAlgError
    GA, GM = 0.5 * (GA + GA.T), 0.5 * (GM + GM.T)
    if not (np.all(np.isfinite(GA)) and np.all(np.isfinite(GM))):
        return None
    try:
        mu = np.linalg.eigvalsh(GM)
        if mu[0] < m * EPS * max(abs(mu[-1]), abs(mu[0])):
            return None
        lam, V = eigh(GA, GM)
    except (LinAlgError, ValueError):
        return None
    if not (np.all(np.isfinite(lam)) and np.all(np.isfinite(V))):
        return None
    return lam, V


def _independent_columns(G):
    """greedy choice of the columns of a Gram matrix that are independent to working precision (pivots of a Cholesky
    factorisation taken in the given order)"""
    from scipy.linalg import solve_triangular
    k = G.shape[0]
    keep, L = [], np.zeros((0, 0))
    for j in range(k):
        if not G[j, j] > 0.0:
            continue
        w = solve_triangular(L, G[keep, j], lower=True) if keep else np.zeros(0)      # row j of the factor
        piv = G[j, j] - w @ w
        if not piv > 16 * k * EPS * G[j, j]:
            continue
        L = np.block([[L, np.zeros((len(keep), 1))], [w[None, :], np.sqrt(piv) * np.ones((1, 1))]])
        keep.append(j)
    return keep


def lobpcg(A, pre, num, mass=None, free=None, X0=None, tol=1e-8, maxit=200, history=True, fuse=False, seed=0):
    """The num <= AMGX_MULTI_MAX smallest eigenpairs of A x = lambda M x on the free dofs.

    A, pre, mass: block operators, objects with apply_block(mv_in, mv_out) (multivector.MatVecMulti(0, dev) and
    multivector.MultMulti(dev) on the device); mass=None is the identity.  free: 0/1 mask of the dofs (None: all free).  X0: the
    start block (a multi-vector of either backend; None: random columns from `seed`, which needs operators that can allocate).
    history=True is LOBPCG (basis [X, W, P]), False PINVIT (basis [X, W]).  fuse: passed to the device adapters
    (False, True, "gs", "gs_block", or "down" / "gs+down" / "gs_block+down" for the fused down pass as well; "gs+f32" / "gs_block+f32"
    on a preconditioner with single-precision Gauss-Seidel images: device.check_fuse).

    Returns (lams, X, info).  Convergence measure per column: res_j = |A x_j - theta_j M x_j| / (|theta_j| |M x_j|); a column
    with res_j <= tol is locked: it stays in the Rayleigh-Ritz basis but gets no new search directions and no operator or
    preconditioner work.  Reaching maxit is not an error.  info: "res" (iterations + 1 rows of num residuals), "locked_at" (the
    iteration at which each column was locked, -1: never), "iterations", "converged", "status" ("converged", "maxit",
    "breakdown"), the safeguard counters "restarts" (P dropped), "joint_orth" ([X, W] orthonormalised as one block),
    "start_replaced" (dependent start columns replaced) and "op_columns" / "pre_columns" / "mass_columns" (columns handed to
    the three operators)."""
    num = int(num)
    if not (1 <= num <= _lib.AMGX_MULTI_MAX):
        raise NgsAMGError(f"lobpcg: num = {num}, need 1 .. AMGX_MULTI_MAX = {_lib.AMGX_MULTI_MAX}")
    if maxit < 0 or not tol > 0:
        raise NgsAMGError("lobpcg: need maxit >= 0 and tol > 0")
    if X0 is None:
        if not hasattr(A, "zeros"):
            raise NgsAMGError("lobpcg: X0 is needed (the operator cannot allocate a multi-vector)")
        X0 = A.zeros(num).randn_like(num, seed)
    if X0.k != num:
        raise NgsAMGError(f"lobpcg: X0 has {X0.k} columns, num = {num}")
    count = {"op": 0, "pre": 0, "mass": 0}

    def opA(X, Y):
        count["op"] += X.k
        _apply(A, X, Y, fuse)
        return Y.Mask(free)

    def opM(X, Y):
        count["mass"] += X.k
        _apply(mass, X, Y, fuse)
        return Y.Mask(free)

    def opC(X, Y):
        count["pre"] += X.k
        _apply(pre, X, Y, fuse)
        return Y.Mask(free)

    has_m = mass is not None
    # one backing store per role: the basis S = [X | W | P] and its images A S, M S (M = I: M S is S)
    S = X0.zeros_like(3 * num)
    AS = X0.zeros_like(3 * num)
    MS = X0.zeros_like(3 * num) if has_m else S
    T = X0.zeros_like(num)                           # target of the combinations that replace X
    Pk, APk = X0.zeros_like(num), X0.zeros_like(num)  # the search directions of the last step (columns p_cols of X)
    MPk = X0.zeros_like(num) if has_m else Pk
    p_cols = []
    info = {"res": [], "locked_at": np.full(num, -1, dtype=np.int64), "iterations": 0, "converged": False, "status": "maxit",
            "restarts": 0, "joint_orth": 0, "start_replaced": 0}

    def finish(status, lams):
        info["status"] = status
        info["converged"] = status == "converged"
        info["res"] = np.array(info["res"]).reshape(-1, num)
        info["op_columns"], info["pre_columns"], info["mass_columns"] = count["op"], count["pre"], count["mass"]
        return np.array(lams, dtype=np.float64), S[0:num].Copy(), info

    X, AX, MX = S[0:num], AS[0:num], MS[0:num]
    X.Assign(X0).Mask(free)
    # start block: M-orthonormal; dependent columns are replaced by random ones
    for attempt in range(3):
        if has_m:
            opM(X, MX)
        if X.Orthonormalize(MX if has_m else None):
            break
        G = X.InnerProduct(MX)
        keep = _independent_columns(0.5 * (G + G.T)) if np.all(np.isfinite(G)) else []
        bad = [j for j in range(num) if j not in keep]
        if not bad or attempt == 2:
            return finish("breakdown", np.full(num, np.nan))
        X.Scatter(bad, X.randn_like(len(bad), seed + 7919 * (attempt + 1)).Mask(free))
        info["start_replaced"] += len(bad)
    opA(X, AX)
    r = _ritz(X.InnerProduct(AX), np.eye(num), num)
    if r is None:
        return finish("breakdown", np.full(num, np.nan))
    theta, V = r
    for v in ([X, AX, MX] if has_m else [X, AX]):
        v.Assign(v.Combine(V))

    locked = np.zeros(num, dtype=bool)
    for it in range(maxit + 1):
        if it > 0 and it % REFRESH == 0:             # recompute the carried products of the columns still iterated
            act = [j for j in range(num) if not locked[j]]
            Xa = X.Gather(act)
            Ya = Xa.zeros_like(len(act))
            AX.Scatter(act, opA(Xa, Ya))
            if has_m:
                MX.Scatter(act, opM(Xa, Ya))
        # residuals R = A X - M X diag(theta), on the free dofs
        R = AX.Copy()
        MX.Combine(np.diag(-theta), out=R, beta=1.0)
        R.Mask(free)
        rn = np.sqrt(np.abs(np.diag(R.InnerProduct(R))))
        mn = np.sqrt(np.abs(np.diag(MX.InnerProduct(MX))))
        with np.errstate(divide="ignore", invalid="ignore"):
            res = rn / (np.abs(theta) * mn)
        info["res"].append(res)
        info["iterations"] = it
        newly = (res <= tol) & ~locked
        info["locked_at"][newly] = it
        locked |= newly
        if locked.all():
            return finish("converged", theta)
        if it == maxit:
            break
        if not np.all(np.isfinite(res)):
            return finish("breakdown", theta)
        act = [j for j in range(num) if not locked[j]]
        na = len(act)
        # W = C R on the active columns, M-orthogonal to X, M-orthonormal
        W, AW, MW = S[num:num + na], AS[num:num + na], MS[num:num + na]
        opC(R.Gather(act), W)
        if has_m:
            X.Combine(-MX.InnerProduct(W), out=W, beta=1.0)
            opM(W, MW)
        else:
            X.Combine(-X.InnerProduct(W), out=W, beta=1.0)
        w_ok = W.Orthonormalize(MW if has_m else None)
        if not w_ok:                                  # no usable new direction: nothing left to improve the basis with
            return finish("breakdown", theta)
        opA(W, AW)                                    # the one operator product of the iteration
        # P: the active ones of the carried directions, M-orthonormalised on their own
        np_ = 0
        if history and p_cols:
            sel = [i for i, j in enumerate(p_cols) if j in act]
            if sel:
                np_ = len(sel)
                P, AP, MP = S[num + na:num + na + np_], AS[num + na:num + na + np_], MS[num + na:num + na + np_]
                P.Assign(Pk.Gather(sel))
                AP.Assign(APk.Gather(sel))
                if has_m:
                    MP.Assign(MPk.Gather(sel))
                if not P.Orthonormalize(MP if has_m else None, carry=[AP]):
                    np_ = 0
                    info["restarts"] += 1
        # Rayleigh-Ritz on [X, W, P]; a failure drops P (a restart), then [X, W] is orthonormalised as one block
        r = None
        while True:
            m = num + na + np_
            B, AB, MB = S[0:m], AS[0:m], MS[0:m]
            GA = B.InnerProduct(AB)
            GM = B.InnerProduct(MB) if has_m else B.InnerProduct(B)
            r = _ritz(GA, GM, m)
            if r is not None:
                break
            if np_ > 0:
                np_ = 0
                info["restarts"] += 1
                continue
            info["joint_orth"] += 1
            if not B.Orthonormalize(MB if has_m else None, carry=[AB]):
                return finish("breakdown", theta)
            r = _ritz(B.InnerProduct(AB), np.eye(m), m)
            if r is None:
                return finish("breakdown", theta)
            break
        lam, V = r
        theta, Cx = lam[:num].copy(), V[:, :num]
        # new X, A X, M X: one combination each of the whole basis; new P: the same without the X block
        Cp = Cx[:, act].copy()
        Cp[:num, :] = 0.0
        for (src, dst, keep) in ((B, X, Pk), (AB, AX, APk)) + (((MB, MX, MPk),) if has_m else ()):
            if history:
                src.Combine(Cp, out=keep[0:na])
            src.Combine(Cx, out=T)
            dst.Assign(T)
        p_cols = list(act) if history else []
    return finish("maxit", theta)
